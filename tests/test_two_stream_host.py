"""CPU-only checks of Spectroscopy.compute_solar_flux: the numpy mirror of its definition
(tests/two_stream_cases.py) against what two-stream theory demands of it, the Rayleigh fit's pins,
that the case tables reach every branch of csrc/twostream.h they are named for, the argument
checks (all raised before anything touches the GPU), the header of the two entries
(include/lbl_amd_twostream.h) against their ctypes signatures, what one call queues on a stand-in engine, and the float64-vs-long-double scan
of the mirror over the case tables that measures E_cpu (printed; two_stream_cases.E_CPU records
it and the GPU tests take their bound from it)."""
import ctypes
import inspect
import json
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, paths
from pylbl_amd import engine as engine_module
from tests import abi_header, sweep_cases as cases, two_stream_cases as ts
from tests import surface_cases as surface
from tests.abi_header import parameters_of
from tests.test_linear_source_host import make_spectroscopy

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd_twostream.h").read_text()
KERNELS = (ROOT / "pylbl_amd" / "csrc" / "twostream.h").read_text()
F64, LD = np.float64, np.longdouble
EPS_LD = float(np.finfo(LD).eps)
ONES = np.ones((3, 5))
GRID_POINTS = 100            # make_spectroscopy's grid


# ---------------------------------------------------------------------------------------------
# The mirror's own properties, in long double.
def columns_of(rng, depth, count, omega=None, g_max=0.9):
    """`count` random columns of `depth` levels as one scatterer per level over an absorber:
    (table [depth, 5] per column stacked as [depth, count, 5], beta [depth, count])."""
    tau_c = 10.**rng.uniform(-3., 1.7, size=(depth, count))
    omega_c = rng.uniform(0.2, 1., size=(depth, count)) if omega is None else \
        np.full((depth, count), omega)
    g_c = rng.uniform(0., g_max, size=(depth, count))
    w_c = omega_c*tau_c
    table = np.stack([np.ones_like(tau_c), np.zeros_like(tau_c), tau_c, w_c, w_c*g_c], axis=-1)
    return table, np.zeros((depth, count))


def solve(kind, table, beta, mu0, albedo, f0=1.):
    inputs = ts.layer_inputs(table, mu0, beta, 0.)
    return ts.adding(kind, ts.layer(kind, inputs), albedo, f0), inputs


@pytest.mark.parametrize("depth", [1, 8, 17])
def test_nothing_is_lost_without_absorption(depth):
    """omega = 1 and A = 1: the net flux is 0 at every interface.  The conservative branch's
    Rdif + Tdif = 1 and Rdir + Tdp + D = 1 hold to a rounding each and adding keeps them: 2000
    long-double roundings leave room for the 1/(1 - Rdif*Rupd) of thick layers under A = 1."""
    rng = np.random.default_rng(depth)
    table, beta = columns_of(rng, depth, 200, omega=1.)
    for mu0 in (1., 0.25, 1e-3):
        got, inputs = solve(LD, table, beta, mu0, 1.)
        assert np.all(inputs["branch"] == ts.CONSERVATIVE_BRANCH)
        net = np.abs(got["up"] - got["down"])
        assert np.all(net <= 2000*EPS_LD), float(net.max())
        assert np.all(np.abs(got["up"][0] - 1.) <= 2000*EPS_LD)


def test_two_halves_make_the_layer():
    """A layer split into two halves gives the same fluxes at its outer interfaces: the
    two-stream solution of a homogeneous layer is a semigroup in its depth.  In long double from
    float64 layer inputs the halves' t, w and gp are the layer's to a float64 rounding, which the
    fluxes see through derivatives of order 1 at these depths: 1e-14."""
    rng = np.random.default_rng(5)
    table, beta = columns_of(rng, 1, 300)
    table[0, :, 2:] = np.minimum(table[0, :, 2:], 20.)
    table[0, :, 3] = 0.9*table[0, :, 2]
    table[0, :, 4] = 0.5*table[0, :, 3]
    half = np.concatenate([table, table], axis=0).copy()
    half[..., 2:] = half[..., 2:]/2.
    for mu0, albedo in ((1., 0.3), (0.25, 0.), (0.6, 1.)):
        whole, inputs = solve(LD, table, beta, mu0, albedo)
        assert np.all(inputs["branch"] == ts.GENERAL)
        split, _ = solve(LD, half, np.zeros((2, 300)), mu0, albedo)
        for q in ts.QUANTITIES:
            assert np.all(np.abs(whole[q][0] - split[q][0]) <= 1e-14), q
            assert np.all(np.abs(whole[q][1] - split[q][2]) <= 1e-14), q


def test_without_scattering_the_beam_and_its_echo_remain():
    """No scatterer and no Rayleigh scattering: w = 0, so direct = F0*prod D_i, nothing diffuse
    comes down, and Rup[0] = A*prod D_i*exp(-2 t_i) (PIFM's diffuse transmittance of an absorber).
    A handful of long-double roundings per level: 40*L."""
    rng = np.random.default_rng(6)
    depth, count = 9, 100
    beta = 10.**rng.uniform(-3., 1., size=(depth, count))
    table = np.zeros((depth, 1, 5))
    table[..., 0] = rng.uniform(0.5, 1.5, size=(depth, 1))
    for mu0, albedo in ((1., 0.3), (0.25, 1.)):
        got, inputs = solve(LD, table, beta, mu0, albedo, f0=0.8)
        assert set(np.unique(inputs["branch"])) == {ts.GENERAL}
        t = inputs["t"].astype(LD)
        beam = np.cumprod(np.exp(-t/LD(mu0)), axis=0)
        bound = 40*depth*EPS_LD
        assert np.all(np.abs(got["direct"][1:] - LD(0.8)*beam) <= bound*LD(0.8)*beam)
        assert got["direct"][0] == pytest.approx(0.8, abs=0.) or np.all(got["direct"][0] == LD(0.8))
        assert np.all(got["diffuse"] == 0.)
        echo = LD(albedo)*beam[-1]*np.prod(np.exp(-2*t), axis=0)
        assert np.all(np.abs(got["rup"][0] - echo) <= bound*echo)
        # At the surface what goes up is A times what comes down.
        assert np.all(np.abs(got["up"][-1] - LD(albedo)*got["down"][-1]) <=
                      bound*got["down"][-1])


def test_general_branch_tends_to_the_conservative_one():
    """Both branches at the same layer differ like (1 - omega): the threshold is continuous."""
    rng = np.random.default_rng(7)
    tau = 10.**rng.uniform(-2., 1., size=200)
    g = rng.uniform(0., 0.9, size=200)
    worst = []
    for delta in (1e-6, 1e-8):
        results = []
        for omega in (1., 1. - delta):
            w_c = omega*tau
            table = np.stack([np.ones(200), np.zeros(200), tau, w_c, w_c*g], axis=-1)[None]
            got, inputs = solve(LD, table, np.zeros((1, 200)), 0.5, 0.3)
            results.append((got, set(np.unique(inputs["branch"]))))
        assert results[0][1] == {ts.CONSERVATIVE_BRANCH} and results[1][1] == {ts.GENERAL}
        worst.append(max(float(np.max(np.abs(results[0][0][q] - results[1][0][q])))
                         for q in ts.QUANTITIES))
    assert worst[0] <= 1e-3 and worst[1] <= 1.1e-2*worst[0]


def test_resonance_guard_is_continuous():
    """Across |1 - k*mu0| = 1e-4 the fluxes move by no more than the guard's own shift of m."""
    inputs = ts.resonance()
    got = ts.mirror(LD, inputs, False)
    for p in range(cases.PATHS):
        mine = inputs.third == p
        d = inputs.d[mine]
        for q in ts.QUANTITIES:
            rows = got[q][2*p:2*p + 2][:, mine]
            for sign in (1., -1.):
                inside = rows[:, d == sign*0.9999e-4]
                outside = rows[:, d == sign*1.0001e-4]
                assert np.all(np.abs(inside - outside) <= 1e-6), (p, q, sign)


# ---------------------------------------------------------------------------------------------
# The Rayleigh fit.
def test_cross_section_pins():
    sigma = paths.rayleigh_cross_section(np.array([1e4/0.5, 1e4/0.55]))
    assert abs(sigma[0] - 6.65e-31) <= 0.01*6.65e-31
    assert abs(sigma[1] - 4.51e-31) <= 0.01*4.51e-31
    nu = ts.rayleigh_grid()
    ours, _ = ts.rayleigh(F64, nu)
    assert np.array_equal(ours, paths.rayleigh_cross_section(nu))
    assert np.all(ours[:2] == 0.) and np.all(ours[2:] > 0.) and np.all(np.isfinite(ours))
    # Both rows of the fit, and the split itself on the short side.
    lam = 1e4/nu[2:]
    assert np.any(lam <= 0.5) and np.any(lam > 0.5) and np.any(lam == 0.5)
    reference, x = ts.rayleigh(LD, nu)
    assert np.all(np.abs(ours.astype(LD) - reference) <= (4*x + 4)*LD(2.**-53)*reference)
    assert paths.K_B == 1.380649e-23


def test_constants_agree():
    for name, row in (("kRayleighShort", paths.RAYLEIGH_SHORT),
                      ("kRayleighLong", paths.RAYLEIGH_LONG)):
        text = re.search(r"%s\[4\] = \{([^}]+)\}" % name, KERNELS).group(1)
        assert tuple(float(x) for x in text.split(",")) == row
    assert paths.RAYLEIGH_SHORT == (3.01577e-28, 3.55212, 1.35579, 0.11563)
    assert paths.RAYLEIGH_LONG == (4.01061e-28, 3.99668, 1.10298e-3, 2.71393e-2)
    assert "kTwoStreamConservative = 1e-10" in KERNELS and ts.CONSERVATIVE == 1e-10
    assert "kTwoStreamResonance = 1e-4" in KERNELS and ts.RESONANCE == 1e-4
    assert "kTwoStreamUpAhead = kPathAhead" in KERNELS and ts.UP_AHEAD == cases.PATH_AHEAD
    assert "kTwoStreamDownAhead = %d" % ts.DOWN_AHEAD in KERNELS
    assert "kRayleighSplit = 0.5" in KERNELS and paths.RAYLEIGH_SPLIT == 0.5


def test_header_docstring_and_kernel_state_the_same_formulas():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    for text in (HEADER, KERNELS, Spectroscopy.compute_solar_flux.__doc__):
        text = squeeze(text)
        for formula in (
                "tau = (tau_a + tau_R) + tau_c", "g2 = (3*(w*(1 - gp)))/4 ; dif = 2*(1 - w)",
                "Rdir = (x + (g3 - g1*mu0)*(-expm1(-t/mu0)))/(1 + x) ; Tdp = (1 - Rdir) - D",
                "den = k*(1 + E2) + g1*o1 ; q = ((1 - x)*(1 + x))*den",
                "Rdir = w*((1 - x)*(a2 + k*g3) - ((1 + x)*(a2 - k*g3))*E2 - "
                "(2*(k*(g3 - a2*m)))*(E*Dm))/q",
                "Ttot = Dm*(1 - w*((1 + x)*(a1 + k*g4) - ((1 - x)*(a1 - k*g4))*E2)/q) + "
                "w*((2*(k*(g4 + a1*m)))*E)/q",
                "Rup[i] = Rdir_i + Tdif_i*((Tdp_i*Rupd[i+1] + D_i*Rup[i+1])*m1)",
                "Td = Tb*Tdp_i + Tdif_i*((Td + (Tb*Rd)*Rdir_i)*m3)"):
            assert formula in text, formula
    # The layer is written once and both kernels call it.
    assert KERNELS.count("TwoStreamLayer two_stream_layer(") == 1
    assert KERNELS.count("= two_stream_layer(") == 2
    assert "path_levels<kTwoStreamUpAhead, kVector>" in KERNELS
    assert "path_levels<kTwoStreamDownAhead, kVector>" in KERNELS
    assert "delta-scaled beam" in squeeze(Spectroscopy.compute_solar_flux.__doc__)
    assert "plane-parallel" in squeeze(Spectroscopy.compute_solar_flux.__doc__)


# ---------------------------------------------------------------------------------------------
# The case tables reach the branches they are named for.
def branches_of(inputs, from_last=False):
    return inputs.layer_inputs(from_last)


def test_case_tables_reach_every_branch():
    ro = ts.rayleigh_only()
    li = branches_of(ro)
    branch, group = li["branch"], ro.group
    # beta = 0 under Rayleigh scattering alone: exactly conservative, w == 1 and k2 == 0.
    zero = branch[:, :, group == 0]
    assert set(np.unique(zero)) == {ts.IDENTITY, ts.CONSERVATIVE_BRANCH}
    conservative = zero == ts.CONSERVATIVE_BRANCH
    assert np.all(li["w"][:, :, group == 0][conservative] == 1.)
    assert np.all(li["k2"][:, :, group == 0][conservative] == 0.)
    # s_l = c_l = 0: the identity, in every column.
    assert np.all(branch[3] == ts.IDENTITY) and np.all(branches_of(ro, True)["branch"][5] ==
                                                       ts.IDENTITY)
    # Both sides of k2*(1 + t*t) = 1e-10, within a factor 30 of it on either side.
    with np.errstate(invalid="ignore"):
        criterion = (li["k2"]*(1. + li["t"]*li["t"]))[:, :, group == 1]
    criterion = criterion[np.isfinite(criterion)]
    assert np.any((criterion > ts.CONSERVATIVE/30.) & (criterion <= ts.CONSERVATIVE))
    assert np.any((criterion > ts.CONSERVATIVE) & (criterion < 30.*ts.CONSERVATIVE))
    assert np.any(branch[:, :, group == 1] == ts.CONSERVATIVE_BRANCH)
    assert np.any(branch[:, :, group == 1] == ts.GENERAL)
    # s*beta >= 800, conservative and thick, omega = 0.
    assert np.all(li["tau"][[0, -1]][:, :, group == 2] >= 800.)
    thick = li["tau"][:, :, group == 4]
    assert np.any(thick > 100.) and np.all(branch[:, :, group == 4] != ts.GENERAL)
    absorbing = li["w"][:, :, group == 5][branch[:, :, group == 5] != ts.IDENTITY]
    assert absorbing.size and np.all(absorbing == 0.)
    assert np.any(ro.solar == 0.)

    cloud = ts.cloud()
    li = branches_of(cloud)
    assert np.any(cloud.omega_c == 0.) and np.any(cloud.omega_c == 1.)
    assert cloud.g_c.max() == 0.9 and np.any(cloud.table[:, 2] == 900.)
    assert np.any(cloud.table[:, 2] == 0.) and np.any(cloud.table[:, 1] == 0.)
    assert np.all(li["tau"][[0, -1]][:, :, cloud.group == 1] >= 800.)
    assert set(np.unique(li["branch"])) >= {ts.CONSERVATIVE_BRANCH, ts.GENERAL}
    assert set(cloud.mu0) >= {1., 1e-3} and set(cloud.albedo) >= {0., 1.}

    res = ts.resonance()
    li = branches_of(res)
    for p in range(cases.PATHS):
        mine = res.third == p
        x = li["x"][:, p][:, mine]
        codes = li["branch"][:, p][:, mine]
        d = res.d[mine]
        for value in ts.RESONANCE_D:
            inside = abs(value) < ts.RESONANCE
            assert np.all(codes[:, d == value] == (ts.GUARDED if inside else ts.GENERAL))
            assert np.all(np.abs((x[:, d == value] - 1.) - value) <= 1e-12), (p, value)
        assert np.any(li["above"][:, p][:, mine][codes == ts.GUARDED])
        assert np.any(~li["above"][:, p][:, mine][codes == ts.GUARDED])
        assert np.all(li["branch"][:, p][:, ~mine] == ts.GENERAL)

    # The shapes: every loop of path_levels for both kernels, both orders, lanes of 1 and 2.
    classes = {cases.depth_class(n, ts.UP_AHEAD) for n in ts.DEPTHS}
    assert classes == {"below", "one batch", "batch and remainder", "batches",
                       "batches and remainder"}
    assert {cases.depth_class(n, ts.DOWN_AHEAD) for n in ts.DEPTHS} == {"one batch", "batches"}
    assert set(ts.DEPTHS) >= {1, 8, 9, 17}
    vector = {cases.layout_is_vector(name, columns)
              for name in cases.LAYOUTS for columns in cases.LAYOUT_COLUMNS}
    assert vector == {True, False}
    assert {w for columns in cases.LAYOUT_COLUMNS for w in cases.lane_widths(columns)} == {1, 2}
    assert any(columns > cases.PATH_THREADS*cases.PATH_WIDTH for columns in cases.LAYOUT_COLUMNS)
    shape = ts.shape_inputs(513, 9, 49)
    codes = np.unique(shape.layer_inputs(True)["branch"])
    assert set(codes) == {ts.IDENTITY, ts.CONSERVATIVE_BRANCH, ts.GENERAL}
    assert set(ts.MU0) == {1., 1e-3, 0.25} and set(ts.ALBEDO) == {1., 0.3, 0.}


def test_float64_mirror_stays_close_to_long_double():
    """E_cpu: the worst |float64 - long double|/F0 over every case table, printed."""
    worst = 0.
    for inputs, from_last in ts.all_cases():
        error, finite = ts.worst_error(inputs, from_last)
        assert finite, inputs.name
        print("%-20s from_last=%-5s worst |difference|/F0 %.3g" % (inputs.name, from_last, error))
        worst = max(worst, error)
    print("E_cpu = %.3g" % worst)
    assert worst <= ts.E_CPU <= ts.E_CPU_CAP == 1e-10
    assert ts.E_CPU <= 2.*worst, "two_stream_cases.E_CPU no longer records the measured value"


# ---------------------------------------------------------------------------------------------
# The requests.
KNOTS = np.array([590., 600., 610.])
CLOUD = dict(scatterer_optical_depth=ONES, scatterer_single_scattering_albedo=0.9*ONES,
             scatterer_asymmetry=0.8*ONES)
BAD = [
    (dict(layer_thickness=np.ones((3, 4))), "shape"),
    (dict(layer_thickness=-ONES), "finite and >= 0"),
    (dict(solar_zenith_cosine=0.), r"\(0, 1\]"),
    (dict(solar_zenith_cosine=1.0001), r"\(0, 1\]"),
    (dict(solar_zenith_cosine=[1., np.nan, 1.]), r"\(0, 1\]"),
    (dict(solar_zenith_cosine=np.ones(5)), "shape"),
    (dict(distance_factor=0.), "distance_factor"),
    (dict(solar_wavenumber=KNOTS), "needs solar_irradiance"),
    (dict(solar_irradiance=-np.ones(GRID_POINTS)), "finite and >= 0"),
    (dict(solar_irradiance=[1., 1.], solar_wavenumber=KNOTS), "one value per knot"),
    (dict(surface="top"), "surface must be"),
    (dict(surface_albedo=1.2), r"\[0, 1\]"),
    (dict(surface_albedo=[0.1, np.nan, 0.3]), r"\[0, 1\]"),
    (dict(surface_albedo=np.ones(4)), "shape"),
    (dict(surface_albedo=[0.1, 0.2], albedo_wavenumber=KNOTS), "shape"),
    (dict(surface_albedo=[0.1, 0.2, 0.3], albedo_wavenumber=[3., 2., 1.]),
     "albedo_wavenumber must be finite and strictly ascending"),
    (dict(rayleigh="yes"), "rayleigh must be"),
    (dict(rayleigh_cross_section=np.ones(GRID_POINTS - 1)), "one value per grid point"),
    (dict(rayleigh_cross_section=-np.ones(GRID_POINTS)), "finite and >= 0"),
    (dict(rayleigh_cross_section=np.full(GRID_POINTS, np.inf)), "finite and >= 0"),
    (dict(rayleigh=False, rayleigh_cross_section=np.ones(GRID_POINTS)), "only used with"),
    (dict(scatterer_optical_depth=ONES), "together or not at all"),
    (dict(scatterer_asymmetry=ONES*0.5, scatterer_optical_depth=ONES), "together or not at all"),
    (dict(CLOUD, scatterer_optical_depth=np.ones((3, 4))), "shape"),
    (dict(CLOUD, scatterer_optical_depth=-ONES), ">= 0"),
    (dict(CLOUD, scatterer_optical_depth=ONES*np.inf), "finite"),
    (dict(CLOUD, scatterer_single_scattering_albedo=1.01*ONES), r"\[0, 1\]"),
    (dict(CLOUD, scatterer_single_scattering_albedo=ONES*np.nan), "finite"),
    (dict(CLOUD, scatterer_asymmetry=ONES), r"\[0, 1\)"),
    (dict(CLOUD, scatterer_asymmetry=-0.1*ONES), r"\[0, 1\)"),
    (dict(quantities="net_flux"), "quantities must be"),
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
    call = dict(layer_thickness=ONES, solar_zenith_cosine=0.5)
    call.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_solar_flux(**call)


def test_rayleigh_and_heating_need_a_physical_atmosphere(monkeypatch):
    untouchable(monkeypatch)
    spec = make_spectroscopy((3, 5))
    spec.atmosphere.pressure = spec.atmosphere.pressure.copy()
    spec.atmosphere.pressure[1, 2] = 0.
    with pytest.raises(ValueError, match="Rayleigh scattering needs pressures"):
        spec.compute_solar_flux(ONES, 0.5)
    with pytest.raises(ValueError, match="heating rates need pressures"):
        spec.compute_solar_flux(ONES, 0.5, rayleigh=False, quantities="heating_rate")
    request = spec._solar_flux_request(ONES, 0.5, None, None, 1., "first", 0., None, False, None,
                                       None, None, None, "upward_flux", None, "reference")
    assert np.all(request.level_table[:, 1:] == 0.)
    spec.atmosphere.pressure[1, 2] = 5e4
    spec.atmosphere.temperature = spec.atmosphere.temperature.copy()
    spec.atmosphere.temperature[0, 0] = 0.
    with pytest.raises(ValueError, match="temperatures"):
        spec.compute_solar_flux(ONES, 0.5)


def test_group_and_instrument_are_not_offered():
    spec = make_spectroscopy((3, 5))
    spec.group = object()
    with pytest.raises(NotImplementedError):
        spec.compute_solar_flux(ONES, 0.5)
    assert "instrument" not in inspect.signature(Spectroscopy.compute_solar_flux).parameters
    assert "solar_path_length" not in inspect.signature(Spectroscopy.compute_solar_flux).parameters


def test_requests_hold_what_the_sweep_needs():
    spec = make_spectroscopy((3, 5))
    thickness = np.arange(1., 16.).reshape(3, 5)
    tau_c = np.linspace(0., 3., 15).reshape(3, 5)
    omega_c, g_c = np.full((3, 5), 0.7), np.linspace(0., 0.9, 15).reshape(3, 5)
    request = spec._solar_flux_request(
        thickness, [1., 0.5, 0.3], None, None, 1.03, "last", [0.1, 0.2, 0.3], None, True, None,
        tau_c, omega_c, g_c, ("heating_rate", "direct_irradiance"), None, "reference")
    assert request.quantities == ("direct_irradiance", "heating_rate")
    table = request.level_table
    assert table.shape == (15, 5) and table.flags.c_contiguous
    assert np.array_equal(table[:, 0], thickness.ravel())
    p, t = spec.atmosphere.pressure.ravel(), spec.atmosphere.temperature.ravel()
    assert np.array_equal(table[:, 1], (p/(paths.K_B*t))*thickness.ravel())
    assert np.array_equal(table[:, 2], tau_c.ravel())
    assert np.array_equal(table[:, 3], (omega_c*tau_c).ravel())
    assert np.array_equal(table[:, 4], ((omega_c*tau_c)*g_c).ravel())
    assert request.scale == paths.SOLAR_SOLID_ANGLE*1.03 and request.rayleigh
    assert request.rayleigh_values is None and request.albedo_knots is None
    assert np.array_equal(request.mu0, [1., 0.5, 0.3])
    sigma = np.linspace(0., 1e-30, GRID_POINTS)
    request = spec._solar_flux_request(
        thickness, 0.25, [1., 2., 0.], KNOTS, 1., "first", [[0.1, 0.2, 0.3]]*3, KNOTS, True,
        sigma, None, None, None, "upward_flux", [600., 600.5], "skip")
    assert np.array_equal(request.rayleigh_values, sigma) and request.albedo.shape == (3, 3)
    assert np.all(request.level_table[:, 2:] == 0.) and request.starts is not None
    bound = inspect.signature(Spectroscopy.compute_solar_flux).parameters
    assert list(bound)[1:] == [
        "layer_thickness", "solar_zenith_cosine", "solar_irradiance", "solar_wavenumber",
        "distance_factor", "surface", "surface_albedo", "albedo_wavenumber", "rayleigh",
        "rayleigh_cross_section", "scatterer_optical_depth",
        "scatterer_single_scattering_albedo", "scatterer_asymmetry", "quantities", "band_edges",
        "remove_pedestal", "range_policy"]
    assert bound["quantities"].default == ("upward_flux", "downward_flux")
    assert bound["surface_albedo"].default == 0. and bound["rayleigh"].default is True
    from pylbl_amd import spectroscopy
    assert spectroscopy.SOLAR_FLUX_QUANTITIES == paths.SOLAR_FLUX_QUANTITIES


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_twostream.h against abi.TWO_STREAM_PROTOTYPES, whole, as
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


def test_header_declares_both_entries_and_ctypes_match():
    from pylbl_amd import abi
    declared = declarations()
    assert list(declared) == list(abi.TWO_STREAM_PROTOTYPES) == \
        ["lbl_rayleigh_row", "lbl_path_two_stream"]
    assert declared["lbl_rayleigh_row"] == [
        "lbl_engine *engine", "int32_t grid", "int64_t columns", "const double *cross_section",
        "double *row", "int32_t flags"]
    sweep = declared["lbl_path_two_stream"]
    assert sweep[:8] == parameters_of("lbl_path_compute")[:8]
    outputs = ["double *%s" % name for name in engine_module.PATH_TWO_STREAM_OUTPUTS]
    assert sweep[8:] == [
        "const double *level_table", "const double *solar_zenith_cosine",
        "const double *solar_row", "const double *rayleigh_row", "const double *albedo_rows",
        "const double *albedo", "int32_t n_bands", "const int64_t *band_start",
        "double *work"] + outputs + ["int32_t flags"]
    # The library exports both, with the table's types set on them; these entries take plain
    # addresses.
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    for name, parameters in declared.items():
        argtypes = abi.TWO_STREAM_PROTOTYPES[name]
        assert len(argtypes) == len(parameters), name
        for argtype, parameter in zip(argtypes, parameters):
            abi_header.check_parameter(argtype, parameter, addresses=True)
        function = getattr(lib, name)
        assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
        assert name not in abi.PROTOTYPES and name not in abi.RESULT_TYPES
    # lbl_amd.h is as it was: the new header includes it and declares nothing of its own twice.
    assert '#include "lbl_amd.h"' in HEADER
    assert not set(declared) & set(abi_header.DECLARATIONS)
    for method in ("rayleigh_row", "path_two_stream"):
        assert callable(getattr(engine_module.Engine, method))


# ---------------------------------------------------------------------------------------------
# The queue.
def argument(line, name):
    return re.search(r"\b%s=([^,)]+)" % name, line).group(1)


def queue_of(spec, engine, limit_rows, **keywords):
    spec.device_output_limit = (8 << 30) if limit_rows is None else limit_rows*surface.ROW_BYTES
    engine.begin()
    result = spec.compute_solar_flux(**keywords)
    return list(engine.log), result


@pytest.mark.parametrize("surface_end", ["first", "last"])
def test_one_call_computes_beta_once_per_run_of_whole_paths(tmp_path, monkeypatch, surface_end):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    quantities = paths.SOLAR_FLUX_QUANTITIES
    with ts.recorded(tmp_path) as (spec, engine):
        # 3 blocks per level and one per interface quantity (4 on the grid): 7 rows a level,
        # 21 a path of three levels.
        for limit, runs in ((None, 1), (42, 1), (41, 2), (21, 2)):
            log, result = queue_of(
                spec, engine, limit, layer_thickness=thickness, solar_zenith_cosine=[0.5, 0.8],
                surface=surface_end, surface_albedo=[[0.2, 0.4], [0.1, 0.3]],
                albedo_wavenumber=[10., 70.], quantities=quantities)
            # Two lines gases: two compute calls per run, each level in exactly one run.
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            sweeps = [line for line in log if line.startswith("path_two_stream(")]
            assert len(sweeps) == runs
            begins = [int(argument(line, "level_begin")) for line in sweeps]
            from_last = surface_end == "first"
            assert begins == sorted(begins, reverse=from_last) and len(set(begins)) == runs
            assert all(begin % 3 == 0 for begin in begins)
            assert {argument(line, "from_last") for line in sweeps} == {str(from_last)}
            # The S row, the sigma row and the albedo rows are filled once, before the first sweep.
            names = [line.split("(")[0] for line in log if line.startswith(
                ("solar_spectrum", "rayleigh_row", "surface_emissivity", "path_two_stream"))]
            assert names == ["solar_spectrum", "rayleigh_row", "surface_emissivity"] + \
                ["path_two_stream"]*runs
            fill = next(line for line in log if line.startswith("rayleigh_row"))
            assert {argument(line, "rayleigh_row") for line in sweeps} == {argument(fill, "row")}
            assert argument(fill, "cross_section") == "None"
            rows = next(line for line in log if line.startswith("surface_emissivity"))
            assert {argument(line, "albedo_rows") for line in sweeps} == {argument(rows, "rows")}
            assert {argument(line, "albedo") for line in sweeps} == {"None"}
            for line in sweeps:
                blocks = {argument(line, name) for name in
                          ("beta", "work", "up_rows", "down_rows", "direct_rows", "diffuse_rows",
                           "top_up_rows", "top_down_rows", "top_direct_rows", "top_diffuse_rows")}
                assert len(blocks) == 10 and "up_mean" not in line
            for q in paths.SOLAR_FLUX_INTERFACE_QUANTITIES:
                assert result[q].shape == (2, 4, 160)
            assert result["heating_rate"].shape == (2, 3, 160)
        # One path does not fit: refused like compute_jacobian.
        with pytest.raises(ValueError, match="does not hold one path"):
            queue_of(spec, engine, 20, layer_thickness=thickness, solar_zenith_cosine=0.5,
                     quantities=quantities)
        # Bands: the sweeps write blocks of the call, the outputs receive their means; without
        # Rayleigh scattering no sigma row is made.
        log, result = queue_of(spec, engine, None, layer_thickness=thickness,
                               solar_zenith_cosine=0.5, surface=surface_end, rayleigh=False,
                               surface_albedo=0.3, band_edges=[20., 30., 60.],
                               quantities=("upward_flux", "heating_rate"))
        sweep, = [line for line in log if line.startswith("path_two_stream(")]
        assert argument(sweep, "band_start") != "None" and "rayleigh_row=None" in sweep
        assert not any(line.startswith("rayleigh_row") for line in log)
        assert argument(sweep, "up_mean") != argument(sweep, "up_rows")
        assert "down_mean" in sweep and "direct_rows" not in sweep and "albedo_rows=None" in sweep
        assert result["upward_flux"].shape == (2, 4, 2)
        assert result["heating_rate"].shape == (2, 3, 2)
        assert np.array_equal(result["band_points"], [40, 120])


def test_existing_calls_queue_what_they_queued(tmp_path):
    """compute_radiance's recorded queues are unchanged, and neither it nor compute_solar
    reaches the new entries."""
    golden = json.loads((ROOT / "tests" / "golden" / "radiance_default_queue.json").read_text())
    got = surface.default_queues(tmp_path)
    assert set(golden) == set(got)
    for name, log in golden.items():
        assert got[name] == log, name
    from tests import solar_cases
    with solar_cases.recorded(tmp_path) as (spec, engine):
        engine.begin()
        spec.compute_solar(np.ones(surface.SHAPE), 0.5)
        spec.compute_radiance(np.ones(surface.SHAPE), boundary_temperature=288.)
        assert not any(line.startswith(("rayleigh_row", "path_two_stream"))
                       for line in engine.log)
