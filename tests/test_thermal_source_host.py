"""CPU-only checks of Spectroscopy.compute_thermal_flux_linear: the weight q of
csrc/twostream_thermal.h's kLinear layer in float64 against long double, that the case tables of
tests/thermal_source_cases.py reach what they are named for, the float64-vs-long-double scan of
the numpy mirror that measures E_cpu (printed; thermal_source_cases.E_CPU records it and the GPU
tests take their bound from it), the mirror against what the linear source demands of it, the
mirror without scatterers against the recurrence of compute_flux(source="linear_in_tau") with one
angle, the header of the entry (include/lbl_amd_thermal_source.h) against its ctypes signature, the
argument checks (all raised before anything touches the GPU) and what one call queues on a
stand-in engine."""
import ctypes
import inspect
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, paths
from pylbl_amd import engine as engine_module
from tests import abi_header, linear_source_cases as ls, sweep_cases as cases
from tests import surface_cases as surface
from tests import thermal_cases as tc, thermal_source_cases as sc
from tests.abi_header import parameters_of
from tests.test_linear_source_host import make_spectroscopy

ROOT = Path(__file__).resolve().parents[1]
HEADER_PATH = ROOT / "include" / "lbl_amd_thermal_source.h"
KERNEL_PATH = ROOT / "pylbl_amd" / "csrc" / "twostream_thermal.h"
F64, LD = np.float64, np.longdouble
ONES = np.ones((3, 5))
INTERFACES = np.linspace(210., 290., 18).reshape(3, 6)


# ---------------------------------------------------------------------------------------------
# The weight.
def test_general_weight_meets_the_long_double_one():
    """q in float64, as the kernel forms it, against q in long double with a longer series below
    Y0 and the direct p above, over y from 1e-8 to 50 and su*t from 1e-6 to 1e3; and the
    long-double q against the plain (1 - T + R)/(su*t) - T where su*t >= 0.05."""
    k, t, su, g1 = sc.weight_samples()
    y, sut = k*t, su*t
    assert y.min() <= 1.1e-8 and y.max() >= 49. and sut.min() <= 1.1e-6 and sut.max() >= 900.
    below = y < sc.Y0
    assert np.any(below) and np.any(~below) and sc.Y0 in y
    low = sc.general_q(F64, k, t, su, g1, below, sc.SERIES_TERMS)
    wide = [a.astype(LD) for a in (k, t, su, g1)]
    high = sc.general_q(LD, *wide, below, sc.REFERENCE_TERMS)
    assert np.all(np.isfinite(low)) and np.all(high > 0.)
    error = np.abs(low.astype(LD) - high)/high
    worst = int(np.argmax(error))
    print("worst relative error of q: %.3g at y = %.3g, su*t = %.3g" % (
        float(error[worst]), y[worst], sut[worst]))
    assert float(error[worst]) <= sc.Q_BOUND == 1.5e-14
    assert sc.Q_ERROR <= sc.Q_BOUND and float(error[worst]) <= sc.Q_ERROR <= 2.*float(
        error[worst]), "thermal_source_cases.Q_ERROR no longer records the measured value"
    # The series and the direct form agree where they meet, and the series is not needed above.
    either = [sc.general_q(LD, *wide, np.full(y.shape, side), sc.REFERENCE_TERMS)
              for side in (True, False)]
    near = (y > 0.4) & (y < 0.6)
    assert np.all(np.abs(either[0] - either[1])[near] <= 1e-16*high[near])
    # The plain form, in long double: its terms reach 2/(su*t) <= 40, eight roundings of 2^-64.
    kk, tt, ss, gg = wide
    with np.errstate(all="ignore"):
        e = np.exp(-(kk*tt))
        o1 = -np.expm1(-(2*(kk*tt)))
        den = kk*(1 + e*e) + gg*o1
        r, tr = ((ss - gg)*o1)/den, (2*(kk*e))/den
        plain = (1 - tr + r)/(ss*tt) - tr
    thick = sut >= 0.05
    gap = float(np.max(np.abs(plain - high)[thick]))
    print("worst |q - plain form| where su*t >= 0.05: %.3g" % gap)
    assert gap <= 40.*8.*2.**-64


def test_general_weight_against_fifty_digits():
    """The thin range, where the plain form has nothing left in long double."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    k, t, su, g1 = (a[:3000] for a in sc.weight_samples(30000))
    low = sc.general_q(F64, k, t, su, g1, k*t < sc.Y0, sc.SERIES_TERMS)
    worst = 0.
    for i in range(k.size):
        kk, tt, ss, gg = (mp.mpf(float(a[i])) for a in (k, t, su, g1))
        e = mp.exp(-kk*tt)
        den = kk*(1 + e*e) + gg*(1 - e*e)
        r, tr = (ss - gg)*(1 - e*e)/den, 2*kk*e/den
        plain = (1 - tr + r)/(ss*tt) - tr
        worst = max(worst, float(abs(mp.mpf(float(low[i])) - plain)/plain))
    print("worst relative error of q against 50 digits: %.3g" % worst)
    assert worst <= sc.Q_BOUND


def test_conservative_weight_joins_the_general_one():
    """At k2*(1 + t*t) = 1e-10 the conservative q, the first-order limit in k, is within
    JOIN_BOUND (relative) of the long-double general q."""
    rng = np.random.default_rng(13)
    count = 20000
    t = 10.**rng.uniform(-3., 1.5, size=count)
    su = rng.uniform(0.3, 2., size=count)
    k2 = tc.CONSERVATIVE/(1. + t*t)
    dif = k2/su
    g1 = (su + dif)/2.
    conservative = ((dif*t)*(1. + (su*t)/3.))/(2.*(1. + g1*t))
    wide = [a.astype(LD) for a in (np.sqrt(k2), t, su, g1)]
    general = sc.general_q(LD, *wide, np.ones(count, dtype=bool), sc.REFERENCE_TERMS)
    gap = float(np.max(np.abs(conservative.astype(LD) - general)/general))
    print("worst relative gap at the threshold: %.3g" % gap)
    assert gap <= sc.JOIN_BOUND == 1e-10
    assert gap <= sc.JOIN_GAP <= 2.*gap, "thermal_source_cases.JOIN_GAP is not the measured value"


def test_clear_weight_is_the_entry_weight_of_the_linear_sweeps():
    """q = a - w of a clear level is radiance.h's u_in, and equals (1 - T)/x - T."""
    x = 10.**np.linspace(-6., 3., 2001)
    inputs = tc.layer_inputs(np.stack([np.ones_like(x), x/1.66, 0.*x, 0.*x, 250. + 0.*x], axis=-1),
                             1.66, np.zeros_like(x))
    assert np.all(inputs["branch"] == tc.CLEAR)
    xs = 1.66*inputs["t"]
    q = sc.weight(F64, inputs)
    assert np.array_equal(q, -np.expm1(-xs) - ls.device_weight(xs))
    wide = xs.astype(LD)
    plain = (-np.expm1(-wide))/wide - np.exp(-wide)
    assert np.all(np.abs(q.astype(LD) - plain) <= 4.*2.**-53)


# ---------------------------------------------------------------------------------------------
# The case tables reach what they are named for.
def test_case_tables_reach_what_they_are_named_for():
    kernels = KERNEL_PATH.read_text()
    assert "kThermalSourceUpAhead = %d;" % sc.UP_AHEAD in kernels
    assert "kThermalSourceDownAhead = %d;" % sc.DOWN_AHEAD in kernels
    assert "kThermalSourceSeriesBelow = 1./2.;" in kernels and sc.Y0 == 0.5
    assert kernels.count("z*(") == 2*(sc.SERIES_TERMS - 1)       # the head's statement, the code
    assert {1, 2, 3, 8, 9, 17} <= set(sc.DEPTHS)
    for ahead in (sc.UP_AHEAD, sc.DOWN_AHEAD):
        assert {1, ahead, ahead + 1, 2*ahead, 2*ahead + 1} <= set(sc.DEPTHS)
    assert set(sc.CLOUD_PLACES) == {"first", "last", "every", "none"}
    for place in sc.CLOUD_PLACES:
        inputs = sc.cloud(place)
        n = inputs.levels_per_path
        cloudy = inputs.cloudy.reshape(cases.PATHS, n)
        expect = {"first": cloudy[:, 0].all() and not cloudy[:, 1:].any(),
                  "last": cloudy[:, -1].all() and not cloudy[:, :-1].any(),
                  "every": cloudy.all(), "none": not cloudy.any()}[place]
        assert expect, place
        li = inputs.layer_inputs(False)
        branch = li["branch"]
        if place == "none":
            assert np.all(branch == tc.CLEAR) and np.all(inputs.table[:, 1:4] == 0.)
            # beta = 0 (the identity layer) and tau = 1e3.
            assert np.any(li["tau"] == 0.)
            assert np.any(np.abs(li["tau"] - 1e3) <= 1e-9) and li["tau"].max() < 1.1e3
            continue
        # omega_c = 1 over beta = 0, and both sides of the conservative threshold within a
        # factor 30 of it, 1 - omega just above it among them.
        assert {tc.CLEAR, tc.CONSERVATIVE_BRANCH, tc.GENERAL} >= set(np.unique(branch))
        assert {tc.CONSERVATIVE_BRANCH, tc.GENERAL} <= set(np.unique(branch))
        order = inputs.order(False).T
        near = (inputs.omega_c[order] == 1.)[:, :, None] & (inputs.group == 1)[None, None, :]
        criterion = (li["k2"]*(1. + li["t"]*li["t"]))[near]
        assert np.any((criterion > tc.CONSERVATIVE/30.) & (criterion <= tc.CONSERVATIVE))
        assert np.any((criterion > tc.CONSERVATIVE) & (criterion < 30.*tc.CONSERVATIVE))
        assert np.any(li["k2"][branch == tc.CONSERVATIVE_BRANCH] == 0.)
    # y crosses Y0 inside a wavefront (64 lanes of two columns), in every level.
    inputs = sc.crossing()
    li = inputs.layer_inputs(True)
    assert np.all(li["branch"] == tc.GENERAL)
    y = np.sqrt(li["k2"])*li["t"]
    below = y[:, :, :128] < sc.Y0
    assert np.all(below.any(axis=2) & (~below).any(axis=2))
    assert len({int(np.argmin(row)) for row in below.reshape(-1, below.shape[2])}) > 3
    # The temperatures: nu = 0, inversions, jumps of 30 K, a path of one temperature, and a
    # surface that is not its interface.
    for inputs in (sc.shape_inputs(131, 9, 2), sc.cloud("every")):
        steps = np.diff(inputs.interfaces, axis=1)
        assert np.any(steps[0] < 0.) and np.any(steps[0] > 0.)
        assert np.all(np.abs(steps[1]) == 30.) and np.any(steps[1] < 0.)
        assert np.all(inputs.interfaces[2] == sc.EQUAL_T)
        assert np.all(inputs.table[2*inputs.levels_per_path:, 4] == sc.EQUAL_T)
        for side in (0, -1):
            assert np.all(inputs.interfaces[:, side] != inputs.surface_t)
        assert inputs.edges.shape == (inputs.levels, 2)
        assert np.array_equal(inputs.edges[1:9, 0], inputs.edges[:8, 1])
    assert sc.shape_inputs(131, 9, 2).nu[0] == 0.
    codes = np.unique(sc.shape_inputs(257, 9, 49).layer_inputs(True)["branch"])
    assert set(codes) == {tc.CLEAR, tc.CONSERVATIVE_BRANCH, tc.GENERAL}


def test_float64_mirror_stays_close_to_long_double():
    """E_cpu: the worst |float64 - long double|/scale over every case table, printed."""
    worst = 0.
    for inputs, from_last in sc.all_cases():
        error, finite = sc.worst_error(inputs, from_last)
        assert finite, inputs.name
        print("%-20s D=%.2f from_last=%-5s worst |difference|/scale %.3g" % (
            inputs.name, inputs.diffusivity, from_last, error))
        worst = max(worst, error)
    print("E_cpu = %.3g" % worst)
    assert worst <= sc.E_CPU <= sc.E_CPU_CAP == 1e-10
    assert sc.E_CPU <= 2.*worst, "thermal_source_cases.E_CPU no longer records the measured value"
    assert sc.FLUX_FLOOR == 1e-13


# ---------------------------------------------------------------------------------------------
# The mirror's own properties, in float64, with bounds in units of E_CPU*scale.
def sources_of(kind, table, d, beta, nu, interfaces):
    """(layers, q, bt, bb) of levels [L, n] under interfaces [L + 1, n]."""
    inputs = tc.layer_inputs(table, d, beta)
    return (tc.layer(kind, inputs), sc.weight(kind, inputs),
            tc.pi_planck(kind, nu, interfaces[:-1]), tc.pi_planck(kind, nu, interfaces[1:]), inputs)


def test_two_halves_with_the_midpoint_source_make_the_layer():
    """A level split into two halves, the Planck value between them (Bt + Bb)/2, leaves the
    fluxes at the outer interfaces unchanged: the source is linear in the layer's depth."""
    from tests.test_thermal_host import clouds_below
    rng = np.random.default_rng(5)
    depth, count = 5, 300
    table = clouds_below(rng, depth, count)
    table[..., 1:3] = np.minimum(table[..., 1:3], 20.)
    beta = 10.**rng.uniform(-4., 0., size=(depth, count))
    nu = rng.uniform(1., 3000., size=count)
    interfaces = rng.uniform(180., 320., size=(depth + 1, count))
    half = np.concatenate([table[:2], table[2:3], table[2:]], axis=0).copy()
    half[2:4, :, :3] = half[2:4, :, :3]/2.
    half_beta = np.concatenate([beta[:2], beta[2:3], beta[2:]], axis=0)
    worst = 0.
    for eps in (1., 0.3):
        layers, q, bt, bb, inputs = sources_of(F64, table, 1.66, beta, nu, interfaces)
        assert {tc.CLEAR, tc.GENERAL} <= set(np.unique(inputs["branch"][2]))
        surface_b = tc.pi_planck(F64, nu, 300.)
        whole = sc.adding(F64, layers, q, bt, bb, eps, surface_b)
        layers, q, _, _, _ = sources_of(F64, half, 1.66, half_beta, nu,
                                        np.zeros((depth + 2, count)) + 250.)
        middle = (bt[2] + bb[2])/2.
        split = sc.adding(F64, layers, q, np.concatenate([bt[:3], middle[None], bt[3:]]),
                          np.concatenate([bb[:2], middle[None], bb[2:]]), eps, surface_b)
        scale = tc.pi_planck(LD, nu, 320.)
        for name in tc.QUANTITIES:
            for i, j in ((0, 0), (2, 2), (3, 4), (5, 6)):
                error = np.abs(whole[name][i].astype(LD) - split[name][j])/scale
                worst = max(worst, float(error.max()))
    print("worst |whole - halves|/scale = %.3g E_cpu" % (worst/sc.E_CPU))
    assert worst <= sc.SPLIT_BOUND*sc.E_CPU


def test_equal_temperatures_give_the_isothermal_mirror_bit_for_bit():
    """dB = 0: both sources are Bt*em.  Path 2 of every case has one temperature at every
    interface and level; all paths of a case flattened to one temperature each too."""
    seen = 0
    for inputs, from_last in sc.all_cases()[::3]:
        for flat in (False, True):
            if flat:
                table = inputs.table.copy()
                table[:, 4] = np.repeat((240., 275., sc.EQUAL_T), inputs.levels_per_path)
                inputs = sc.Inputs(inputs.name, inputs.nu, inputs.beta, table,
                                   np.repeat(np.array([[240.], [275.], [sc.EQUAL_T]]),
                                             inputs.levels_per_path + 1, axis=1),
                                   inputs.surface_t, inputs.emissivity, inputs.diffusivity)
            got = sc.mirror(F64, inputs, from_last)
            expect = tc.mirror(F64, inputs.isothermal(), from_last)
            n = inputs.levels_per_path
            rows = slice(0 if flat else 2*n, 3*n)
            for name in tc.NAMES + ("u", "rs"):
                part = slice(0 if flat else 2, 3) if name.startswith("top_") else rows
                assert np.array_equal(got[name][part].view(np.uint64),
                                      expect[name][part].view(np.uint64)), (inputs.name, name)
                seen += 1
    assert seen > 100


def test_a_thick_clear_layer_sends_down_its_lower_face_less_the_gradient():
    """Under a clear layer of tau = 1e3 the flux leaving its surface-side face is Bb - dB/x."""
    rng = np.random.default_rng(17)
    count = 400
    nu = rng.uniform(1., 3000., size=count)
    interfaces = rng.uniform(180., 320., size=(2, count))
    worst = 0.
    for d in (1.66, 2., 1.):
        table = np.stack([np.ones(count), np.full(count, 1e3), np.zeros(count), np.zeros(count),
                          np.full(count, 250.)], axis=-1)[None]
        got, inputs = sc.column(F64, table, d, np.zeros((1, count)), nu, interfaces, 0.3, 300.)
        assert np.all(inputs["branch"] == tc.CLEAR)
        bt, bb = (tc.pi_planck(LD, nu, interfaces[i]) for i in (0, 1))
        expect = bb - (bb - bt)/(LD(d)*LD(1e3))
        scale = np.maximum(bt, bb)
        worst = max(worst, float(np.max(np.abs(got["down"][1].astype(LD) - expect)/scale)))
    print("worst |down - (Bb - dB/x)|/scale = %.3g E_cpu" % (worst/sc.E_CPU))
    assert worst <= sc.THICK_BOUND*sc.E_CPU


# ---------------------------------------------------------------------------------------------
# Without scatterers: compute_flux's linear recurrence with the one angle mu = 1/D, w = 1.
def plain_fluxes(kind, inputs, from_last):
    """tests/test_thermal_host.py's plain_fluxes with tests/linear_source_cases.py's sweep."""
    n = inputs.levels_per_path
    mu = np.array([1./inputs.diffusivity])
    weight = np.array([1.])
    lengths = inputs.table[:, :1]/mu
    down = ls.sweep_flux(kind, inputs.nu, inputs.beta, lengths, weight, inputs.edges, n, from_last)
    start, _ = cases.surface_start(kind, inputs.nu, inputs.surface_t, inputs.emissivity,
                                   down.total, down.total_mag)
    up = ls.sweep_flux(kind, inputs.nu, inputs.beta, lengths, weight, inputs.edges, n,
                       not from_last, start)
    order = inputs.order(from_last)
    below = np.zeros_like(up.flux)
    below[order[:, :-1]] = up.flux[order[:, 1:]]
    below[order[:, -1]] = kind(cases.FLUX_PI)*start
    return {"down": down.flux, "up": below, "top_up": up.flux[order[:, 0]]}


def clear_inputs(depth, seed, d):
    problem = cases.Problem(131, depth, seed=seed)
    zeros = np.zeros(problem.levels)
    table = np.stack([problem.thickness, zeros, zeros, zeros, problem.temperature], axis=1)
    interfaces, table = sc.interfaces_for(table, depth, seed)
    return sc.Inputs("clear", problem.nu, problem.beta, table, interfaces, tc.SURFACE_T,
                     tc.EMISSIVITY, d)


@pytest.mark.parametrize("d", [1.66, 2.])
@pytest.mark.parametrize("from_last", [False, True])
def test_without_scatterers_it_is_the_linear_flux_recurrence_with_one_angle(d, from_last):
    """Within PLAIN_ROUNDINGS*2^-53*(L + 1)*scale (thermal_source_cases.py derives the count)."""
    worst = 0.
    for depth, seed in ((1, 1), (9, 2), (17, 3)):
        inputs = clear_inputs(depth, seed, d)
        got = sc.mirror(F64, inputs, from_last)
        expect = plain_fluxes(F64, inputs, from_last)
        bound = LD(sc.PLAIN_ROUNDINGS*2.**-53*(depth + 1))
        for name, value in expect.items():
            scale = got["scale"] if name == "top_up" else sc.per_level(inputs, got["scale"])
            error = np.abs(got[name].astype(LD) - value.astype(LD))
            lit = scale > 0.
            worst = max(worst, float(np.max(error[lit]/(bound*scale[lit]))))
            assert np.all(error <= bound*scale), (depth, name)
    print("D = %g, from_last = %s: worst error / bound %.3g" % (d, from_last, worst))
    assert sc.PLAIN_ROUNDINGS == 24.


# ---------------------------------------------------------------------------------------------
# The statements of the definition.
def test_header_docstring_design_and_kernel_state_the_same_formulas():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    design = (ROOT / "DESIGN.md").read_text()
    section = design[design.index("## 25."):]
    kernels = KERNEL_PATH.read_text()
    for text in (HEADER_PATH.read_text(), kernels, Spectroscopy.compute_thermal_flux_linear.__doc__,
                 section):
        text = squeeze(text)
        for formula in sc.FORMULAS:
            assert formula in text, formula
    for formula in tc.FORMULAS:
        if not formula.startswith(("S = ", "U[i] = ", "Dn = ")):
            assert formula in squeeze(HEADER_PATH.read_text()), formula
    # One layer, one adding step and one pair of kernels serve both sources: the layer is written
    # once and called once, each of its results is assigned once per branch (no second copy to
    # drift), and nothing of the separate linear-source files is left.
    assert kernels.count("ThermalLayer thermal_layer(") == kernels.count(" thermal_layer(") == 1
    assert kernels.count("thermal_layer<kLinear>(") == kernels.count("thermal_layer<") == 1
    for member in ("y.r = ", "y.t = ", "y.em = ", "y.q = "):
        assert kernels.count(member) == 3, member
    assert len(re.findall(r"if constexpr \(kLinear\)\s*\{?\s*y\.q = ", kernels)) == 3
    assert kernels.count("void thermal_through(") == 1
    assert kernels.count("thermal_through(v.clear, y, out, back, flux[i], refl[i]);") == 1
    assert kernels.count("thermal_through(") == 2
    assert kernels.count("__global__") == 2 and kernels.count(".through(l, c, k, b, ") == 2
    csrc = ROOT / "pylbl_amd" / "csrc"
    for path in csrc.iterdir():
        for gone in ("thermal_source_layer", "thermal_source_through", "PathThermalSource",
                     "ThermalSourceLayer"):
            assert gone not in path.read_text(), (path.name, gone)
    assert not (csrc / "twostream_thermal_source.h").exists()
    assert not (csrc / "thermal_source_entry.inc").exists()
    assert "kLinear ? kThermalSourceUpAhead : kThermalUpAhead" in kernels
    assert "path_levels<kAhead, kVector>" in kernels
    assert "path_levels<kThermalDownAhead, kVector>" in kernels
    assert "kThermalSourceDownAhead == kThermalDownAhead" in kernels
    for reused in ("thermal_level(", "thermal_columns<kVector>(", "thermal_pi_planck(",
                   "thermal_surface<kVector>(", "thermal_interface<kVector>("):
        assert reused in kernels, reused


def test_signature_and_defaults():
    signature = inspect.signature(Spectroscopy.compute_thermal_flux_linear).parameters
    assert list(signature)[1:] == [
        "layer_thickness", "surface_temperature", "interface_temperature", "surface_emissivity",
        "emissivity_wavenumber", "surface", "diffusivity", "scatterer_optical_depth",
        "scatterer_single_scattering_albedo", "scatterer_asymmetry", "quantities", "band_edges",
        "remove_pedestal", "range_policy"]
    empty = inspect.Parameter.empty
    defaults = {name: p.default for name, p in signature.items() if p.default is not empty}
    assert defaults == dict(
        surface_emissivity=1., emissivity_wavenumber=None, surface="first", diffusivity=1.66,
        scatterer_optical_depth=None, scatterer_single_scattering_albedo=None,
        scatterer_asymmetry=None, quantities=("upward_flux", "downward_flux"), band_edges=None,
        remove_pedestal=None, range_policy="reference")
    assert not {"instrument", "source", "group"} & set(signature)
    # compute_thermal_flux is as it was.
    old = inspect.signature(Spectroscopy.compute_thermal_flux).parameters
    assert [name for name in signature if name != "interface_temperature"] == list(old)


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_thermal_source.h against abi.THERMAL_SOURCE_PROTOTYPES, whole, as
# tests/test_abi_host.py compares lbl_amd.h with abi.PROTOTYPES.
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
    header = HEADER_PATH.read_text()
    declared = declarations(header)
    name = "lbl_path_thermal_two_stream_source"
    assert list(declared) == list(abi.THERMAL_SOURCE_PROTOTYPES) == [name]
    # lbl_path_thermal_two_stream's arguments with edge_temperature behind level_table.
    old = declarations((ROOT / "include" / "lbl_amd_thermal.h").read_text())[
        "lbl_path_thermal_two_stream"]
    assert old[9] == "const double *level_table"
    assert declared[name] == old[:10] + ["const double *edge_temperature"] + old[10:]
    assert "const double *edge_temperature" in parameters_of("lbl_path_flux_source")
    assert abi.THERMAL_SOURCE_PROTOTYPES[name] == \
        abi.THERMAL_PROTOTYPES["lbl_path_thermal_two_stream"][:10] + [ctypes.c_void_p] + \
        abi.THERMAL_PROTOTYPES["lbl_path_thermal_two_stream"][10:]
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    argtypes = abi.THERMAL_SOURCE_PROTOTYPES[name]
    assert len(argtypes) == len(declared[name])
    for argtype, parameter in zip(argtypes, declared[name]):
        abi_header.check_parameter(argtype, parameter, addresses=True)
    function = getattr(lib, name)
    assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
    for table in (abi.PROTOTYPES, abi.TWO_STREAM_PROTOTYPES, abi.THERMAL_PROTOTYPES,
                  abi.KDIST_PROTOTYPES, abi.RESULT_TYPES):
        assert name not in table
    assert '#include "lbl_amd.h"' in header
    assert not set(declared) & set(abi_header.DECLARATIONS)
    assert callable(engine_module.Engine.path_thermal_two_stream_source)


# ---------------------------------------------------------------------------------------------
# The requests.
KNOTS = np.array([590., 600., 610.])
CLOUD = dict(scatterer_optical_depth=ONES, scatterer_single_scattering_albedo=0.9*ONES,
             scatterer_asymmetry=0.8*ONES)


def changed(row, column, value):
    out = INTERFACES.copy()
    out[row, column] = value
    return out


BAD = [
    (dict(interface_temperature=None), "needs interface_temperature"),
    (dict(interface_temperature=np.full((3, 5), 250.)), "shape"),
    (dict(interface_temperature=np.full((3, 7), 250.)), "shape"),
    (dict(interface_temperature=np.full(6, 250.)), "shape"),
    (dict(interface_temperature=changed(1, 2, np.nan)), "finite and > 0"),
    (dict(interface_temperature=changed(0, 0, np.inf)), "finite and > 0"),
    (dict(interface_temperature=changed(2, 5, 0.)), "finite and > 0"),
    (dict(interface_temperature=changed(2, 5, -3.)), "finite and > 0"),
    (dict(layer_thickness=np.ones((3, 4))), "shape"),
    (dict(layer_thickness=-ONES), "finite and >= 0"),
    (dict(surface_temperature=0.), "finite and > 0"),
    (dict(surface_temperature=[288., np.nan, 288.]), "finite and > 0"),
    (dict(surface_temperature=np.full(5, 288.)), "shape"),
    (dict(surface_emissivity=1.2), r"\[0, 1\]"),
    (dict(surface_emissivity=np.ones(4)), "shape"),
    (dict(surface_emissivity=[0.1, 0.2, 1.3], emissivity_wavenumber=KNOTS), r"\[0, 1\]"),
    (dict(surface_emissivity=[0.1, 0.2, 0.3], emissivity_wavenumber=[3., 2., 1.]),
     "emissivity_wavenumber must be finite and strictly ascending"),
    (dict(surface="top"), "surface must be"),
    (dict(diffusivity=0.9), r"diffusivity must be one number in \[1, 2\]"),
    (dict(diffusivity=np.nan), "diffusivity"),
    (dict(scatterer_optical_depth=ONES), "together or not at all"),
    (dict(CLOUD, scatterer_optical_depth=-ONES), ">= 0"),
    (dict(CLOUD, scatterer_single_scattering_albedo=1.01*ONES), r"\[0, 1\]"),
    (dict(CLOUD, scatterer_asymmetry=ONES), r"\[0, 1\)"),
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
    call = dict(layer_thickness=ONES, surface_temperature=288., interface_temperature=INTERFACES)
    call.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_thermal_flux_linear(**call)


def test_group_is_not_offered_and_the_message_names_the_method():
    spec = make_spectroscopy((3, 5))
    spec.group = object()
    with pytest.raises(NotImplementedError, match="compute_thermal_flux_linear"):
        spec.compute_thermal_flux_linear(ONES, 288., INTERFACES)
    with pytest.raises(NotImplementedError, match="compute_thermal_flux does"):
        spec.compute_thermal_flux(ONES, 288.)


def test_requests_hold_what_the_sweep_needs():
    spec = make_spectroscopy((3, 5))
    thickness = np.arange(1., 16.).reshape(3, 5)
    arguments = ([1., 0.5, 0.], None, "last", 2., None, None, None, ("upward_flux",), None,
                 "reference")
    request = spec._thermal_flux_linear_request(thickness, [288., 270., 300.], INTERFACES,
                                                *arguments)
    plain = spec._thermal_flux_request(thickness, [288., 270., 300.], *arguments)
    assert plain.edge_temperature is None
    for name in plain._fields:
        if name != "edge_temperature":
            assert np.array_equal(getattr(request, name), getattr(plain, name)), name
    edges = request.edge_temperature
    assert edges.shape == (15, 2) and edges.flags.c_contiguous and edges.dtype == F64
    assert np.array_equal(edges, ls.edge_table(INTERFACES))
    assert np.array_equal(edges, paths._edge_temperatures("linear_in_tau", INTERFACES, (3, 5)))
    # T_l of the table is the level temperature still: it sets beta, the kernels do not read it.
    assert np.array_equal(request.level_table[:, 4], spec.atmosphere.temperature.ravel())


# ---------------------------------------------------------------------------------------------
# The queue.
def argument(line, name):
    return re.search(r"\b%s=([^,)]+)" % name, line).group(1)


def queue_of(spec, engine, limit_rows, method, **keywords):
    spec.device_output_limit = (8 << 30) if limit_rows is None else limit_rows*surface.ROW_BYTES
    engine.begin()
    engine.edge_tables = []
    result = getattr(spec, method)(**keywords)
    return list(engine.log), result


@pytest.mark.parametrize("surface_end", ["first", "last"])
def test_one_call_queues_the_new_entry_with_its_rows_of_the_edge_table(tmp_path, monkeypatch,
                                                                      surface_end):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    interfaces = surface.interfaces()
    edges = ls.edge_table(interfaces)
    quantities = paths.THERMAL_FLUX_QUANTITIES
    common = dict(layer_thickness=thickness, surface_temperature=[288., 270.],
                  surface=surface_end, surface_emissivity=[[0.2, 0.4], [0.1, 0.3]],
                  emissivity_wavenumber=[10., 70.], diffusivity=2., quantities=quantities)
    new, old = "path_thermal_two_stream_source(", "path_thermal_two_stream("
    with sc.recorded(tmp_path) as (spec, engine):
        for limit, runs in ((None, 1), (30, 1), (29, 2), (15, 2)):
            log, result = queue_of(spec, engine, limit, "compute_thermal_flux_linear",
                                   interface_temperature=interfaces, **common)
            # beta is computed once per run: two lines gases, two compute calls per run.
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            sweeps = [line for line in log if line.startswith(new)]
            assert len(sweeps) == runs and not any(line.startswith(old) for line in log)
            begins = [int(argument(line, "level_begin")) for line in sweeps]
            from_last = surface_end == "first"
            assert begins == sorted(begins, reverse=from_last) and len(set(begins)) == runs
            assert {argument(line, "from_last") for line in sweeps} == {str(from_last)}
            assert {argument(line, "diffusivity") for line in sweeps} == {"2.0"}
            # Every run passes its own rows of the edge table, and together they are the table.
            assert [begin for begin, _ in engine.edge_tables] == begins
            rows = 6//runs
            for begin, table in engine.edge_tables:
                assert np.array_equal(table, edges[begin:begin + rows])
            names = [line.split("(")[0] for line in log if line.startswith(
                ("surface_emissivity", "path_thermal_two_stream"))]
            assert names == ["surface_emissivity"] + [new[:-1]]*runs
            for line in sweeps:
                blocks = {argument(line, name) for name in
                          ("beta", "work", "up_rows", "down_rows", "top_up_rows", "top_down_rows")}
                assert len(blocks) == 6 and "up_mean" not in line
            for q in ("upward_flux", "downward_flux"):
                assert result[q].shape == (2, 4, 160)
            assert result["heating_rate"].shape == (2, 3, 160)
            assert result["source"] == "linear_in_tau"
            # compute_thermal_flux queues what it queued: the old entry alone, with the same
            # arguments but the edge table, and no mark on its result.
            before, plain = queue_of(spec, engine, limit, "compute_thermal_flux", **common)
            assert not any(line.startswith(new) for line in before) and not engine.edge_tables
            assert "source" not in plain
            assert sum(line.startswith("compute(") for line in before) == 2*runs
            was = [line for line in before if line.startswith(old)]
            assert len(was) == runs
            for one, other in zip(was, sweeps):
                assert "edge_temperature" not in one
                other = re.sub(r"\bedge_temperature=[^,)]+, ", "", other.replace(new, old))
                assert one == other
        with pytest.raises(ValueError, match="does not hold one path"):
            queue_of(spec, engine, 14, "compute_thermal_flux_linear", layer_thickness=thickness,
                     surface_temperature=288., interface_temperature=interfaces,
                     quantities=quantities)
        log, result = queue_of(spec, engine, None, "compute_thermal_flux_linear",
                               layer_thickness=thickness, surface_temperature=288.,
                               interface_temperature=interfaces, surface=surface_end,
                               surface_emissivity=0.3, band_edges=[20., 30., 60.],
                               quantities="upward_flux")
        sweep, = [line for line in log if line.startswith(new)]
        assert argument(sweep, "band_start") != "None" and "emissivity_rows=None" in sweep
        assert argument(sweep, "up_mean") != argument(sweep, "up_rows")
        assert "top_up_mean" in sweep and "down_rows" not in sweep
        assert result["upward_flux"].shape == (2, 4, 2) and result["source"] == "linear_in_tau"
    # The isothermal recorder knows nothing of the new entry, and compute_thermal_flux needs
    # nothing else.
    with tc.recorded(tmp_path) as (spec, engine):
        assert not hasattr(engine, "path_thermal_two_stream_source")
        log, _ = queue_of(spec, engine, None, "compute_thermal_flux", **common)
        assert sum(line.startswith(old) for line in log) == 1
