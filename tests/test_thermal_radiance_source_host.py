"""CPU-only checks of Spectroscopy.compute_thermal_radiance_linear: the float64-vs-long-double scan
of the numpy mirror of tests/thermal_radiance_source_cases.py over its case tables that measures
E_cpu (printed; thermal_radiance_source_cases.E_CPU records it and the GPU tests take their bound
from it), the mirror against what the transfer equation demands of it (each bound beside what was
measured), its two bit-for-bit anchors -- compute_thermal_radiance's mirror under one temperature
on all-cloudy paths, compute_radiance's linear recurrence without scatterers --, the statements of
the definition, the header of the entry (include/lbl_amd_thermal_radiance_source.h) against its
ctypes signature, the argument checks (all raised before anything touches the GPU) and what one
call queues on a stand-in engine."""
import ctypes
import inspect
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, paths
from pylbl_amd import engine as engine_module
from tests import abi_header, linear_source_cases as ls, sweep_cases as cases
from tests import scatterer_radiance_cases as spectral_cases
from tests import surface_cases as surface
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_radiance_source_cases as vc
from tests import thermal_source_cases as sc
from tests.abi_header import parameters_of
from tests.test_linear_source_host import make_spectroscopy
from tests.test_thermal_radiance_host import BAD as VIEW_BAD
from tests.test_thermal_radiance_host import argument, quadrature, untouchable
from tests.test_thermal_source_host import INTERFACES, changed

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd_thermal_radiance_source.h").read_text()
KERNELS = (ROOT / "pylbl_amd" / "csrc" / "thermal_radiance_source.h").read_text()
DESIGN = (ROOT / "DESIGN.md").read_text()
F64, LD = np.float64, np.longdouble
ONES = np.ones((3, 5))


# ---------------------------------------------------------------------------------------------
# E_cpu, and what the tables hold.
def test_float64_mirror_stays_close_to_long_double():
    """E_cpu: the worst |float64 - long double|/scale over every case table, printed."""
    worst = 0.
    for inputs, mu, from_last in vc.all_cases():
        error, finite = vc.worst_error(inputs, mu, from_last)
        assert finite, inputs.name
        print("%-20s D=%.2f from_last=%-5s worst |difference|/scale %.3g" % (
            inputs.name, inputs.diffusivity, from_last, error))
        worst = max(worst, error)
    print("E_cpu = %.3g" % worst)
    assert worst <= vc.E_CPU
    assert vc.E_CPU <= 2.*worst, "thermal_radiance_source_cases.E_CPU no longer records the value"
    assert vc.FLOOR == 1e-13 == rc.FLOOR


def test_case_tables_are_those_of_sections_25_and_27():
    assert vc.MU == (1., 0.6, 0.05)
    names = [inputs.name for inputs, _ in vc.value_cases()]
    assert {"pole", "deep", "no cloud", "y across y0", "cloud at every"} <= set(names)
    codes = set()
    for inputs, mu, _ in vc.all_cases():
        assert inputs.columns <= 8193 and inputs.levels_per_path <= 17
        # Path 0 has inversions, path 1 jumps by 30 K per level, path 2 has one temperature; no
        # surface temperature is the surface interface's.
        assert np.all(np.abs(np.diff(inputs.interfaces[1])) == 30.)
        assert np.all(inputs.interfaces[2] == sc.EQUAL_T)
        n = inputs.levels_per_path
        assert np.all(inputs.table[2*n:, 4] == sc.EQUAL_T)
        assert not np.any(inputs.surface_t[:, None] == inputs.interfaces[:, [0, -1]])
        codes |= set(np.unique(inputs.layer_inputs(False)["branch"]))
    assert any(np.any(np.diff(inputs.interfaces[0]) < 0.) and np.any(np.diff(inputs.interfaces[0])
               > 0.) for inputs, _, _ in vc.all_cases())
    assert codes == {tc.CLEAR, tc.CONSERVATIVE_BRANCH, tc.GENERAL}
    pole = vc.pole()
    assert pole.k*pole.mu[0] == 1. and abs(pole.k*pole.mu[1] - 1. - 1e-9) < 1e-15
    assert abs(pole.k*pole.mu[2] - 1. + 1e-9) < 1e-15
    assert "kThermalViewSourceAhead = %d;" % vc.VIEW_AHEAD in KERNELS
    a = vc.VIEW_AHEAD
    assert {1, a, a + 1, 2*a, 2*a + 1} <= set(tc.DEPTHS)


# ---------------------------------------------------------------------------------------------
# The mirror's own properties.
def test_closed_forms_match_quadrature_of_the_source():
    """C of both cloudy branches, with its term (2*(a*c))*Em, against Gauss-Legendre quadrature
    of J's bracket within a level with f+- carrying +-c, in long double, relative to |u1| + |d0| +
    |c|: k*mu = 1 exactly and 1 +- 1e-9, k*t = 1000 with t/mu = 20, and random levels.  And the
    thermal term Bt*Em + dB*(Em - lw) against the quadrature of B(tau), relative to |Bt| + |Bb|."""
    rng = np.random.default_rng(12)
    one, two = LD(1.), LD(2.)
    worst = thermal = 0.
    general = [(1.25, 0.8, 3.), (1.25, 0.8*(1. + 1e-9), 3.), (1.25, 0.8*(1. - 1e-9), 3.),
               (50., 1., 20.), (2., 0.5, 1e-3), (1.9, 1., 40.)]
    general += [(rng.uniform(0.05, 2.), rng.uniform(0.05, 1.), 10.**rng.uniform(-3., 1.5))
                for _ in range(40)]
    assert general[0][0]*general[0][1] == 1. and general[3][0]*general[3][2] == 1000.
    for k, mu, t in general:
        k, mu, t = LD(k), LD(mu), LD(t)
        gamma, a = LD(rng.uniform(0., 0.99)), LD(rng.uniform(0., 0.7))
        u1, d0, c = (LD(rng.uniform(-1., 1.)) for _ in range(3))
        em = -np.expm1(-t/mu)
        closed, p, q, _ = rc.general_c(LD, k, gamma, t, mu, a, u1, d0)
        closed = closed + (two*(a*c))*em
        expect = quadrature(
            t, mu, a, lambda tau: p*np.exp(-k*(t - tau)) + gamma*q*np.exp(-k*tau) + c,
            lambda tau: gamma*p*np.exp(-k*(t - tau)) + q*np.exp(-k*tau) - c)
        assert np.isfinite(closed)
        worst = max(worst, float(abs(closed - expect)/(abs(u1) + abs(d0) + abs(c))))
    for _ in range(40):
        g1, mu, t = LD(rng.uniform(0.2, 2.)), LD(rng.uniform(0.05, 1.)), LD(10.**rng.uniform(-4., 2.))
        a, u1, d0, c = (LD(rng.uniform(-1., 1.)) for _ in range(4))
        a = abs(a)*LD(0.7)
        em = -np.expm1(-t/mu)
        closed, n = rc.conservative_c(LD, g1, t, mu, a, u1, d0)
        closed = closed + (two*(a*c))*em
        expect = quadrature(t, mu, a, lambda tau: u1 - g1*n*(t - tau) + c,
                            lambda tau: d0 + g1*n*tau - c)
        worst = max(worst, float(abs(closed - expect)/(abs(u1) + abs(d0) + abs(c))))
        # The thermal term: int_0^t B(tau) exp(-tau/mu) dtau/mu with B on its line in tau is the
        # bracket of f+ = f- = B/2 under a = 0.
        bt, bb = LD(rng.uniform(0., 1.)), LD(rng.uniform(0., 1.))
        lw = ls.weight(LD, t/mu)
        term = bt*em + (bb - bt)*(em - lw)
        line = lambda tau: (bt + (bb - bt)*tau/t)/two                   # noqa: E731
        expect = quadrature(t, mu, LD(0.), line, line)
        thermal = max(thermal, float(abs(term - expect)/(bt + bb)))
    del one
    print("worst |C - quadrature|/(|u1| + |d0| + |c|) = %.3g; thermal term %.3g" % (worst, thermal))
    assert worst <= vc.QUADRATURE_BOUND and thermal <= vc.QUADRATURE_BOUND


def test_the_internal_solution_reproduces_the_flux_it_did_not_use():
    """f+ at a level's space-side face, P*E + Gamma*Q + c (conservative: u1 - x*N + c), is up[i] -
    pi*Bt: the level's solution was fixed by up[i+1] and down[i] alone.  In long double on
    long-double fluxes of the linear source, relative to pi*scale + |c|: u1 and d0 carry -+c, which
    in a thin level under a 30 K jump is a thousand times pi*scale, and what is left is rounding
    of numbers of that size (general) or what the k = 0 layer leaves out of them (conservative)."""
    worst = {tc.GENERAL: 0., tc.CONSERVATIVE_BRANCH: 0.}
    pi = LD(cases.FLUX_PI)
    for inputs in (vc.with_view(tc.cloud("every"), 52), vc.pole(), vc.shape_inputs(67, 5, 9)):
        for from_last in (False, True):
            fluxes = sc.mirror(LD, inputs, from_last)
            order = inputs.order(from_last)
            li = inputs.layer_inputs(from_last)
            g1, g2, k, _ = rc.scalars(LD, li)
            size = pi*vc.scale(inputs)
            space = 1 if from_last else 0
            for i in range(inputs.levels_per_path):
                here = {name: (value[i] if isinstance(value, np.ndarray) and value.ndim == 3
                               else value) for name, value in li.items()}
                bt = vc.face_planck(LD, inputs, order[:, i], space)
                bb = vc.face_planck(LD, inputs, order[:, i], 1 - space)
                shift, _ = vc.source_shift(LD, here, bt, bb)
                u1 = (fluxes["up"][order[:, i]] - pi*bb) - shift
                top = fluxes["up"][order[:, i - 1]] if i > 0 else fluxes["top_up"]
                d0 = ((fluxes["down"][order[:, i - 1]] if i > 0 else LD(0.)) - pi*bt) + shift
                t = li["t"][i].astype(LD)
                gamma = g2[i]/(g1[i] + k[i])
                _, p, q, e = rc.general_c(LD, k[i], gamma, t, LD(1.), LD(0.), u1, d0)
                _, n = rc.conservative_c(LD, g1[i], t, LD(1.), LD(0.), u1, d0)
                with np.errstate(all="ignore"):
                    got = np.where(li["branch"][i] == tc.GENERAL, p*e + gamma*q,
                                   u1 - (g1[i]*t)*n) + shift
                for code in worst:
                    cloudy = (li["branch"][i] == code) & (size > 0.)
                    if np.any(cloudy):
                        error = (np.abs(got - (top - pi*bt))/(size + np.abs(shift)))[cloudy]
                        worst[code] = max(worst[code], float(error.max()))
    print("worst |f+(0) - (up[i] - pi*Bt)|/(pi*scale + |c|): general %.3g, conservative %.3g" % (
        worst[tc.GENERAL], worst[tc.CONSERVATIVE_BRANCH]))
    assert 0. < worst[tc.GENERAL] <= vc.TOP_BOUND
    assert 0. < worst[tc.CONSERVATIVE_BRANCH] <= vc.TOP_BOUND_CONSERVATIVE <= tc.CONSERVATIVE


def single_column(kind, table, d, beta, nu, faces, eps, surface_t, mu):
    """The radiance of independent columns [count] through levels [L, count, 5] in the order space
    -> surface with the float64 Planck values `faces` [L + 1, count] at their interfaces, on the
    float64 fluxes of thermal_source_cases.adding."""
    li = tc.layer_inputs(table, d, beta)
    pi64 = F64(cases.FLUX_PI)
    fluxes = sc.adding(F64, tc.layer(F64, li), sc.weight(F64, li), pi64*faces[:-1], pi64*faces[1:],
                       eps, tc.pi_planck(F64, nu, np.asarray(surface_t, dtype=F64)))
    depth = table.shape[0]
    one, pi = kind(1.), kind(cases.FLUX_PI)
    eps = kind(eps)
    rad = eps*cases.planck(kind, nu, surface_t) + (one - eps)*(fluxes["down"][depth].astype(kind)/pi)
    for i in range(depth - 1, -1, -1):
        here = {name: (value[i] if isinstance(value, np.ndarray) and value.ndim == 2 else value)
                for name, value in li.items()}
        down0 = fluxes["down"][i] if i > 0 else np.zeros_like(fluxes["down"][0])
        rad = vc.level(kind, here, mu, faces[i].astype(kind), faces[i + 1].astype(kind),
                       fluxes["up"][i + 1], down0, rad)
    return rad, li


def test_two_halves_make_the_level():
    """A level split into two halves, the Planck value of the face between them on the level's
    line in tau (its halves have half of t each: the mean of Bt and Bb), leaves the radiance
    unchanged."""
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
    faces = cases.planck(F64, nu[None, :], rng.uniform(180., 320., size=(depth + 1, count)))
    half = np.concatenate([table[:2], table[2:3], table[2:]], axis=0).copy()
    half[2:4, :, :3] = half[2:4, :, :3]/2.
    half_beta = np.concatenate([beta[:2], beta[2:3], beta[2:]], axis=0)
    middle = faces[2] + (faces[3] - faces[2])/2.
    half_faces = np.concatenate([faces[:3], middle[None], faces[3:]], axis=0)
    scale = cases.planck(LD, nu, 320.)
    worst = 0.
    for eps in (1., 0.3):
        for mu in (1., 0.6, 0.05):
            whole, li = single_column(F64, table, 1.66, beta, nu, faces, eps, 300., mu)
            assert {tc.CLEAR, tc.GENERAL} <= set(np.unique(li["branch"][2]))
            split, _ = single_column(F64, half, 1.66, half_beta, nu, half_faces, eps, 300., mu)
            worst = max(worst, float(np.max(np.abs(whole.astype(LD) - split)/scale)))
    print("worst |whole - halves|/scale = %.3g E_cpu" % (worst/vc.E_CPU))
    assert worst <= vc.SPLIT_BOUND*vc.E_CPU


def test_one_temperature_gives_the_isothermal_bits_on_all_cloudy_paths():
    """dB = 0 and c = 0: where every level of a path is cloudy and every interface, every level
    and nothing else has one temperature, the float64 mirror has the bits of section 27's.  A
    clear level agrees to roundings only (the two clear lines differ)."""
    checked = 0
    for inputs in (vc.pole(), vc.with_view(tc.cloud("every"), 52), vc.deep()):
        n = inputs.levels_per_path
        assert np.all(inputs.table[2*n:, 2] > 0.)
        for from_last in (False, True):
            linear = vc.mirror(F64, inputs, inputs.mu if hasattr(inputs, "mu") else vc.MU,
                               from_last)
            plain = rc.mirror(F64, inputs.isothermal(),
                              inputs.mu if hasattr(inputs, "mu") else rc.MU, from_last)
            for name in ("radiance", "brightness_temperature"):
                assert np.array_equal(linear[name][2].view(np.uint64),
                                      plain[name][2].view(np.uint64)), (inputs.name, name)
            # The paths with gradients differ.
            assert not np.array_equal(linear["radiance"][1], plain["radiance"][1])
            checked += 1
    assert checked == 6
    # Clear levels above a cloud: per clear level Bb*(A - lw), Bt*lw and their sum stand where
    # B*A stood, four roundings of at most scale.
    inputs = sc.cloud("last")
    linear = vc.mirror(F64, inputs, vc.MU, False)
    plain = rc.mirror(F64, inputs.isothermal(), rc.MU, False)
    gap = np.abs(linear["radiance"][2].astype(LD) - plain["radiance"][2])
    assert np.all(gap <= LD(4.*inputs.levels_per_path*2.**-53)*linear["scale"][2])


@pytest.mark.parametrize("from_last", [False, True])
def test_without_scatterers_it_is_compute_radiance_linear_bit_for_bit(from_last):
    """No scatterers, eps = 1 and mu = 1: the float64 mirror has the bits of
    lbl_path_radiance_source's recurrence from B(T_s), swept surface -> space."""
    for depth, seed in ((1, 1), (9, 2), (17, 3)):
        problem = cases.Problem(131, depth, seed=seed)
        zeros = np.zeros(problem.levels)
        table = np.stack([problem.thickness, zeros, zeros, zeros, problem.temperature], axis=1)
        interfaces = ls.interfaces_for(problem, seed)
        inputs = sc.Inputs("clear", problem.nu, problem.beta, table, interfaces, tc.SURFACE_T,
                           np.ones(3))
        got = vc.mirror(F64, inputs, np.ones(3), from_last)["radiance"]
        # The surface lies behind level 0 with from_last: the view sweeps towards the last level.
        start = cases.boundary_start(F64, problem.nu, inputs.surface_t, np.ones(3))
        expect, _ = ls.sweep_radiance(F64, problem.nu, problem.beta, problem.thickness,
                                      inputs.edges, depth, not from_last, start)
        last = inputs.order(from_last)[:, 0]
        assert np.array_equal(got.view(np.uint64), expect[last].view(np.uint64)), depth


def test_reversing_the_gradient_moves_the_radiance_towards_the_exit_face():
    """One thick cloudy level (t about 20, w about 0.5) over a black surface at its mean
    temperature: with the space-side face at 280 K and the other at 220 K the viewer sees more
    than the isothermal level at 250 K gives, with the faces exchanged less, and the step between
    the two is most of the step of B between the faces, and less than it."""
    count = 40
    nu = np.linspace(400., 1400., count)
    table = np.zeros((1, count, 5))
    table[...] = [1., 20., 10., 0.6, 250.]
    beta = np.zeros((1, count))
    warm, cold = cases.planck(F64, nu, 280.), cases.planck(F64, nu, 220.)
    level_b = cases.planck(F64, nu, 250.)
    moves = []
    for mu in vc.MU:
        up_warm, _ = single_column(F64, table, 1.66, beta, nu, np.stack([warm, cold]), 1., 250., mu)
        up_cold, _ = single_column(F64, table, 1.66, beta, nu, np.stack([cold, warm]), 1., 250., mu)
        same, _ = single_column(F64, table, 1.66, beta, nu, np.stack([level_b, level_b]), 1., 250.,
                                mu)
        assert np.all(up_warm > same) and np.all(same > up_cold), mu
        moves.append(float(np.min((up_warm - up_cold)/(warm - cold))))
    # A cloud that scatters half of what it intercepts is no black body: the step stays below B's.
    assert all(0.5 < move < 1. for move in moves), moves


# ---------------------------------------------------------------------------------------------
# The statements of the definition.
def test_header_docstring_design_and_kernel_state_the_same_formulas():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    section = DESIGN[DESIGN.index("## 31."):]
    for text in (HEADER, KERNELS, Spectroscopy.compute_thermal_radiance_linear.__doc__, section):
        text = squeeze(text)
        for formula in vc.FORMULAS:
            assert formula in text, formula
    assert "path_levels<kThermalViewSourceAhead, kVector>" in KERNELS
    new = inspect.signature(Spectroscopy.compute_thermal_radiance_linear).parameters
    old = inspect.signature(Spectroscopy.compute_thermal_radiance).parameters
    assert list(new)[:4] == ["self", "layer_thickness", "surface_temperature",
                             "interface_temperature"]
    assert new["interface_temperature"].default is inspect.Parameter.empty
    # Every other argument is compute_thermal_radiance's, in its order and with its defaults.
    assert [name for name in new if name != "interface_temperature"] == list(old)
    for name, parameter in old.items():
        assert new[name].default == parameter.default and new[name].kind == parameter.kind, name
    assert new["view_zenith_cosine"].default == 1.
    assert new["diffusivity"].default == 1.66 == paths.DIFFUSIVITY
    # The other two are as they were, and the spectral one goes on refusing the argument.
    assert "interface_temperature" not in old
    assert "interface_temperature" not in inspect.signature(
        Spectroscopy.compute_thermal_radiance_spectral).parameters
    # The existing kernels are as they were: the new header only includes them.
    assert '#include "thermal_radiance.h"' in KERNELS
    assert "kLinear" not in (ROOT / "pylbl_amd" / "csrc" / "thermal_radiance.h").read_text()


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_thermal_radiance_source.h against
# abi.THERMAL_RADIANCE_SOURCE_PROTOTYPES, whole.
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


def test_header_declares_the_entry_and_ctypes_match():
    from pylbl_amd import abi
    declared = declarations(HEADER)
    name = "lbl_path_thermal_radiance_source"
    assert list(declared) == list(abi.THERMAL_RADIANCE_SOURCE_PROTOTYPES) == [name]
    # lbl_path_thermal_radiance's arguments with edge_temperature behind level_table.
    plain = declarations((ROOT / "include" / "lbl_amd_thermal_radiance.h").read_text())
    plain = plain["lbl_path_thermal_radiance"]
    assert plain[:9] == parameters_of("lbl_path_flux")[:9]
    assert plain[9] == "const double *level_table"
    assert declared[name] == plain[:10] + ["const double *edge_temperature"] + plain[10:]
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    argtypes = abi.THERMAL_RADIANCE_SOURCE_PROTOTYPES[name]
    assert len(argtypes) == len(declared[name])
    for argtype, parameter in zip(argtypes, declared[name]):
        abi_header.check_parameter(argtype, parameter, addresses=True)
    function = getattr(lib, name)
    assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
    for table in (abi.PROTOTYPES, abi.TWO_STREAM_PROTOTYPES, abi.THERMAL_PROTOTYPES,
                  abi.THERMAL_SOURCE_PROTOTYPES, abi.KDIST_PROTOTYPES, abi.SCATTERER_PROTOTYPES,
                  abi.THERMAL_RADIANCE_PROTOTYPES, abi.SOLAR_RADIANCE_PROTOTYPES,
                  abi.SCATTERER_RADIANCE_PROTOTYPES, abi.RESULT_TYPES):
        assert name not in table
    assert '#include "lbl_amd.h"' in HEADER
    assert not set(declared) & set(abi_header.DECLARATIONS)
    assert callable(engine_module.Engine.path_thermal_radiance_source)


# ---------------------------------------------------------------------------------------------
# The requests.
BAD = [
    (dict(interface_temperature=None), "needs interface_temperature"),
    (dict(interface_temperature=np.full((3, 5), 250.)), "shape"),
    (dict(interface_temperature=np.full((3, 7), 250.)), "shape"),
    (dict(interface_temperature=np.full(6, 250.)), "shape"),
    (dict(interface_temperature=changed(1, 2, np.nan)), "finite and > 0"),
    (dict(interface_temperature=changed(0, 0, np.inf)), "finite and > 0"),
    (dict(interface_temperature=changed(2, 5, 0.)), "finite and > 0"),
    (dict(interface_temperature=changed(2, 5, -3.)), "finite and > 0"),
] + VIEW_BAD


@pytest.mark.parametrize("keywords, match", BAD)
def test_bad_arguments_are_refused_before_the_gpu(monkeypatch, keywords, match):
    untouchable(monkeypatch)
    spec = make_spectroscopy((3, 5))
    call = dict(layer_thickness=ONES, surface_temperature=288., interface_temperature=INTERFACES)
    call.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_thermal_radiance_linear(**call)


def test_bands_and_instrument_exclude_each_other_and_group_is_not_offered(monkeypatch):
    untouchable(monkeypatch)
    from pylbl_amd.instrument import Instrument
    spec = make_spectroscopy((3, 5))
    instrument = Instrument.gaussian(np.array([600.2, 600.4]), 0.1)
    with pytest.raises(ValueError, match="band_edges or instrument, not both"):
        spec.compute_thermal_radiance_linear(ONES, 288., INTERFACES, band_edges=[600., 600.5],
                                             instrument=instrument)
    with pytest.raises(TypeError):
        spec.compute_thermal_radiance_spectral(
            ONES, 288., np.array([590., 610.]), np.ones((3, 5, 2)), np.ones((3, 5, 2)),
            np.zeros((3, 5, 2)), interface_temperature=INTERFACES)
    spec.group = object()
    with pytest.raises(NotImplementedError, match="compute_thermal_radiance_linear"):
        spec.compute_thermal_radiance_linear(ONES, 288., INTERFACES)
    with pytest.raises(NotImplementedError, match="compute_thermal_radiance does"):
        spec.compute_thermal_radiance(ONES, 288.)


def test_requests_hold_what_the_sweep_needs():
    spec = make_spectroscopy((3, 5))
    thickness = np.arange(1., 16.).reshape(3, 5)
    arguments = ([1., 0.5, 0.05], [1., 0.5, 0.], None, "last", 2., None, None, None,
                 ("brightness_temperature", "radiance"), None, None, "reference")
    request = spec._thermal_radiance_linear_request(thickness, [288., 270., 300.], INTERFACES,
                                                    *arguments)
    plain = spec._thermal_radiance_request(thickness, [288., 270., 300.], *arguments)
    assert plain.edge_temperature is None and type(request) is type(plain)
    for name in plain._fields:
        if name != "edge_temperature":
            assert np.array_equal(getattr(request, name), getattr(plain, name)), name
    edges = request.edge_temperature
    assert edges.shape == (15, 2) and edges.flags.c_contiguous and edges.dtype == F64
    assert np.array_equal(edges, ls.edge_table(INTERFACES))
    assert np.array_equal(edges, paths._edge_temperatures("linear_in_tau", INTERFACES, (3, 5)))
    # T_l of the table is the level temperature still: it sets beta, the kernels do not read it.
    assert np.array_equal(request.level_table[:, 4], spec.atmosphere.temperature.ravel())
    assert np.array_equal(request.mu, [1., 0.5, 0.05])


# ---------------------------------------------------------------------------------------------
# The queue.
def queue_of(spec, engine, limit_rows, method, **keywords):
    spec.device_output_limit = (8 << 30) if limit_rows is None else limit_rows*surface.ROW_BYTES
    engine.begin()
    engine.edge_tables, engine.view_edge_tables = [], []
    result = getattr(spec, method)(**keywords)
    return list(engine.log), result


@pytest.mark.parametrize("surface_end", ["first", "last"])
def test_one_call_queues_both_source_entries_with_the_runs_edge_rows(tmp_path, monkeypatch,
                                                                    surface_end):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    interfaces = surface.interfaces()
    edges = ls.edge_table(interfaces)
    both = ("radiance", "brightness_temperature")
    common = dict(layer_thickness=thickness, surface_temperature=[288., 270.],
                  view_zenith_cosine=[1., 0.4], surface=surface_end,
                  surface_emissivity=[[0.2, 0.4], [0.1, 0.3]], emissivity_wavenumber=[10., 70.],
                  diffusivity=2., quantities=both)
    flux_new, view_new = "path_thermal_two_stream_source(", "path_thermal_radiance_source("
    flux_old, view_old = "path_thermal_two_stream(", "path_thermal_radiance("
    with vc.recorded(tmp_path) as (spec, engine):
        # 5 blocks per level: 15 rows a path of three levels.
        for limit, runs in ((None, 1), (30, 1), (29, 2), (15, 2)):
            log, result = queue_of(spec, engine, limit, "compute_thermal_radiance_linear",
                                   interface_temperature=interfaces, **common)
            # Two lines gases: two compute calls per run, beta once per run.
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            names = [line.split("(")[0] for line in log if line.startswith(
                ("surface_emissivity", "path_thermal"))]
            assert names == ["surface_emissivity"] + [flux_new[:-1], view_new[:-1]]*runs
            fluxes = [line for line in log if line.startswith(flux_new)]
            views = [line for line in log if line.startswith(view_new)]
            from_last = surface_end == "first"
            begins = [int(argument(line, "level_begin")) for line in views]
            assert begins == sorted(begins, reverse=from_last) and len(set(begins)) == runs
            assert all(begin % 3 == 0 for begin in begins)
            # Both entries of a run receive the run's rows of the edge table.
            rows = 6//runs
            assert [begin for begin, _ in engine.edge_tables] == begins
            assert [begin for begin, _ in engine.view_edge_tables] == begins
            for begin, table in engine.edge_tables + engine.view_edge_tables:
                assert np.array_equal(table, edges[begin:begin + rows])
            for flux, view in zip(fluxes, views):
                for name in ("beta", "level_begin", "up_rows", "down_rows", "from_last",
                             "diffusivity", "emissivity_rows", "emissivity", "asynchronous",
                             "edge_temperature"):
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
            assert result["source"] == "linear_in_tau"
            # compute_thermal_radiance queues what it queued: the old entries alone, with the
            # same arguments but the edge table, and no mark on its result.
            before, plain = queue_of(spec, engine, limit, "compute_thermal_radiance", **common)
            assert not any(line.startswith((flux_new, view_new)) for line in before)
            assert not engine.edge_tables and not engine.view_edge_tables
            assert "source" not in plain
            was = [line for line in before if line.startswith(("path_thermal",))]
            now = [line for line in log if line.startswith(("path_thermal",))]
            assert len(was) == len(now) == 2*runs
            for one, other in zip(was, now):
                assert "edge_temperature" not in one
                other = other.replace(flux_new, flux_old).replace(view_new, view_old)
                assert one == re.sub(r"\bedge_temperature=[^,)]+, ", "", other)
        # One path does not fit.
        with pytest.raises(ValueError, match="does not hold one path"):
            queue_of(spec, engine, 14, "compute_thermal_radiance_linear",
                     layer_thickness=thickness, surface_temperature=288.,
                     interface_temperature=interfaces)
        # Bands: the sweep writes a block of the call, the output receives its means.
        log, result = queue_of(spec, engine, None, "compute_thermal_radiance_linear",
                               layer_thickness=thickness, surface_temperature=288.,
                               interface_temperature=interfaces, surface=surface_end,
                               surface_emissivity=0.3, band_edges=[20., 30., 60.])
        view, = [line for line in log if line.startswith(view_new)]
        assert argument(view, "band_start") != "None" and "emissivity_rows=None" in view
        assert argument(view, "radiance_mean") != argument(view, "radiance_rows")
        assert "brightness_rows" not in view
        assert result["radiance"].shape == (2, 2) and result["source"] == "linear_in_tau"
    # The recorders of the grey and the spectral call know nothing of the new entry, and those
    # calls need nothing else.
    with spectral_cases.recorded(tmp_path, rc.RadianceRecorder) as (spec, engine):
        assert not hasattr(engine, "path_thermal_radiance_source")
        assert not hasattr(engine, "path_thermal_two_stream_source")
        log, _ = queue_of(spec, engine, None, "compute_thermal_radiance", **common)
        assert sum(line.startswith(view_old) for line in log) == 1
    with spectral_cases.recorded(tmp_path) as (spec, engine):
        assert not hasattr(engine, "path_thermal_radiance_source")
        shape = surface.SHAPE + (2,)
        log, result = queue_of(
            spec, engine, None, "compute_thermal_radiance_spectral", layer_thickness=thickness,
            surface_temperature=288., scatterer_wavenumber=[10., 70.],
            scatterer_optical_depth=np.ones(shape),
            scatterer_single_scattering_albedo=np.full(shape, 0.5),
            scatterer_asymmetry=np.full(shape, 0.3))
        names = [line.split("(")[0] for line in log if line.startswith("path_thermal")]
        assert names == ["path_thermal_two_stream_spectral", "path_thermal_radiance_spectral"]
        assert "source" not in result


def test_existing_calls_do_not_reach_the_new_entry(tmp_path):
    with vc.recorded(tmp_path) as (spec, engine):
        engine.begin()
        spec.compute_thermal_flux(np.ones(surface.SHAPE), 288.)
        spec.compute_thermal_flux_linear(np.ones(surface.SHAPE), 288., surface.interfaces())
        spec.compute_thermal_radiance(np.ones(surface.SHAPE), 288.)
        spec.compute_radiance(np.ones(surface.SHAPE), boundary_temperature=288.)
        assert any(line.startswith("path_thermal_two_stream_source") for line in engine.log)
        assert not any(line.startswith("path_thermal_radiance_source") for line in engine.log)
