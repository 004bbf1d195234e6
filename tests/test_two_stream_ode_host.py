"""CPU-only checks of the two-stream layers and columns against the two-stream equations
themselves (tests/two_stream_ode_cases.py: a long-double solver of the equations that knows none
of the closed forms): that solver against 60-digit mpmath; every long-double mirror
(tests/two_stream_cases.py, tests/thermal_cases.py, tests/thermal_source_cases.py) against it,
layer by layer and column by column, by the branch the mirror takes, over the mirrors' own case
tables and over the tables of the GPU tests; DESIGN section 25's conservative em against the
estimate given there; the resonance guard measured alone; and that the tables the GPU tests hold
to the tight bound have no element in the guard and keep the float64 mirrors within their E_CPU.

Every measured figure is printed, and recorded as a constant of tests/two_stream_ode_cases.py that
must satisfy measured <= CONSTANT <= 2*measured."""
import functools

import numpy as np
import pytest

from tests import scatterer_cases as spectral
from tests import thermal_cases as tc
from tests import thermal_source_cases as tsc
from tests import two_stream_cases as ts
from tests import two_stream_ode_cases as ode

F64, LD = np.float64, np.longdouble
ROUNDING = LD(ode.REFERENCE_BOUND)


def recorded(what, measured, constant):
    """The 2x rule of a constant that records a measured figure."""
    print("%s: measured %.3g, recorded %.3g" % (what, measured, constant))
    assert measured <= constant <= 2.*measured, \
        "two_stream_ode_cases: %s no longer records the measured %.3g" % (what, measured)


def worst_by(classes, count, error, into, names):
    """into[names[i]] = the worst error where classes == i, for each i < count."""
    for index in range(count):
        chosen = classes == index
        if np.any(chosen):
            into[names[index]] = max(into[names[index]], float(np.max(error[chosen])))


# ---------------------------------------------------------------------------------------------
# The mirrors against the reference.
SOLAR_LAYER_NAMES = {ts.IDENTITY: "identity", ts.CONSERVATIVE_BRANCH: "conservative",
                     ts.GENERAL: "general", ts.GUARDED: "guarded"}
THERMAL_LAYER_NAMES = {tc.CLEAR: "clear", tc.CONSERVATIVE_BRANCH: "conservative",
                       tc.GENERAL: "general"}


def relative(error, scale):
    """error/scale where scale > 0; where it is 0 the two must agree exactly."""
    assert np.all(np.isfinite(error))
    dark = scale == 0.
    assert np.all(error[dark] == 0.)
    return np.where(dark, 0., error/np.where(dark, 1., scale))


def solar_deviation(inputs, from_last):
    """(per layer element [L, PATHS, columns], per column [PATHS, columns]) of |long-double
    mirror - reference|, in units of F0, and the layer inputs."""
    li = inputs.layer_inputs(from_last)
    solved = ode.solar_layer(li)
    layers = np.max([np.abs(a - b) for a, b in zip(ts.layer(LD, li), solved)], axis=0)
    assert np.all(np.isfinite(layers))
    mirror = ts.mirror(LD, inputs, from_last)
    reference = ode.solar_reference(inputs, from_last, solved)
    f0 = reference["f0"].astype(LD)
    n = inputs.levels_per_path
    columns = np.zeros(f0.shape, dtype=LD)
    for q in ts.QUANTITIES:
        top = relative(np.abs(mirror["top_" + q] - reference["top_" + q]), f0)
        below = relative(np.abs(mirror[q] - reference[q]), np.repeat(f0, n, axis=0))
        columns = np.maximum(columns, np.maximum(top, np.max(below.reshape(ode.PATHS, n, -1),
                                                            axis=1)))
    return layers, columns, li


def thermal_deviation(inputs, from_last):
    """The same of a thermal_source_cases.Inputs with either source: {linear: (layers, columns)},
    the layer inputs and |em - reference|; in units of B = 1 (layers: R, T and em; with the
    linear source S_up and S_dn under (Bt, Bb) = (0, 1) and (1, 0)) and of the scale (columns)."""
    li = inputs.layer_inputs(from_last)
    r, t, em = tc.layer(LD, li)
    q = tsc.weight(LD, li)
    solved = ode.thermal_layer(li)
    ref_r, ref_t, ref_em, up1, dn1 = solved
    pairs = {False: [(r, ref_r), (t, ref_t), (em, ref_em)],
             True: [(q, up1), (em - q, dn1), (em - q, ref_em - up1), (q, ref_em - dn1)]}
    n = inputs.levels_per_path
    out = {}
    for linear in (False, True):
        layers = np.max([np.abs(a - b) for a, b in pairs[linear]], axis=0)
        assert np.all(np.isfinite(layers))
        mirror = tsc.mirror(LD, inputs, from_last) if linear else \
            tc.mirror(LD, inputs.isothermal(), from_last)
        reference = ode.thermal_reference(inputs, from_last, linear, solved)
        scale = reference["scale"]
        assert np.array_equal(scale, mirror["scale"])
        columns = np.zeros(scale.shape, dtype=LD)
        for name in tc.QUANTITIES:
            top = relative(np.abs(mirror["top_" + name] - reference["top_" + name]), scale)
            below = relative(np.abs(mirror[name] - reference[name]), np.repeat(scale, n, axis=0))
            columns = np.maximum(columns, np.maximum(
                top, np.max(below.reshape(ode.PATHS, n, -1), axis=1)))
        out[linear] = layers, columns
    return out, li, np.abs(em - ref_em)


def own_solar_tables():
    return [(inputs, from_last) for inputs in ode.tight_solar_tables() + ode.guard_tables()
            for from_last in (False, True)]


def own_thermal_tables():
    return [(inputs, from_last) for inputs in ode.thermal_tables() for from_last in (False, True)]


@functools.lru_cache(maxsize=None)
def solar_measured():
    """{"layer": {...}, "column": {...} (the mirrors' tables), "tables": {...} (the GPU tests')}."""
    out = {"layer": dict.fromkeys(ode.SOLAR_LAYER, 0.),
           "column": dict.fromkeys(ode.SOLAR_COLUMN, 0.),
           "tables": dict.fromkeys(ode.SOLAR_TABLES, 0.)}
    for which, table in (("column", ts.all_cases()), ("tables", own_solar_tables())):
        for inputs, from_last in table:
            layers, columns, li = solar_deviation(inputs, from_last)
            worst_by(li["branch"], 4, layers, out["layer"], SOLAR_LAYER_NAMES)
            worst_by(ode.solar_column_class(li), 3, columns, out[which],
                     ode.SOLAR_CLASSES)
    return out


@functools.lru_cache(maxsize=None)
def thermal_measured():
    """{linear: solar_measured's dict}, and of the conservative em (worst error, worst fraction of
    section 25's estimate, elements counted).  The mirrors' tables are thermal_source_cases' for
    both sources: they are thermal_cases' own with interface temperatures beside them."""
    out = {linear: {"layer": dict.fromkeys(ode.THERMAL_LAYER, 0.),
                    "column": dict.fromkeys(ode.THERMAL_COLUMN, 0.),
                    "tables": dict.fromkeys(ode.THERMAL_TABLES, 0.)} for linear in (False, True)}
    worst, fraction, elements = 0., 0., 0
    for which, table in (("column", tsc.all_cases()), ("tables", own_thermal_tables())):
        for inputs, from_last in table:
            both, li, em_error = thermal_deviation(inputs, from_last)
            for linear, (layers, columns) in both.items():
                worst_by(li["branch"], 3, layers, out[linear]["layer"], THERMAL_LAYER_NAMES)
                worst_by(ode.thermal_column_class(li), 3, columns, out[linear][which],
                         ode.THERMAL_CLASSES)
            chosen = li["branch"] == tc.CONSERVATIVE_BRANCH
            if np.any(chosen):
                error = em_error[chosen]
                estimate = (li["k2"]*li["t"]*li["t"]/2.)[chosen].astype(LD)
                # The criterion itself: k2*t*t/2 <= k2*(1 + t*t)/2 <= 5e-11.
                assert np.all(estimate <= 5e-11)
                assert np.all(error <= estimate + ROUNDING)
                worst = max(worst, float(np.max(error)))
                large = estimate > 1e-14
                fraction = max(fraction, float(np.max(error[large]/estimate[large], initial=0.)))
                elements += int(np.count_nonzero(large))
    out["em"] = worst, fraction, elements
    return out


def check_recorded(title, measured, constants):
    for name in constants:
        recorded("%s, %s" % (title, name), measured[name], constants[name])


def test_solar_mirror_against_the_equations_by_branch():
    """The general branch and the identity differ from the equations by rounding alone, the
    conservative one by what its cut allows, the guarded one by the guard's 1e-5."""
    measured = solar_measured()
    check_recorded("SOLAR_LAYER", measured["layer"], ode.SOLAR_LAYER)
    check_recorded("SOLAR_COLUMN", measured["column"], ode.SOLAR_COLUMN)
    check_recorded("SOLAR_TABLES", measured["tables"], ode.SOLAR_TABLES)
    # Where the formulas claim to be exact they are: rounding of the two long-double routes.
    assert ode.SOLAR_LAYER["identity"] == 0.
    # Next to the guard the quotient by (1 - x)*(1 + x) amplifies the mirror's own rounding by up
    # to 1e4: 64*2^-64/1e-4 = 3.5e-14 (two_stream_cases.resonance() has columns 1e-8 outside it).
    near_guard = 64.*2.**-64/ode.GUARD
    assert ode.SOLAR_LAYER["general"] <= near_guard and ode.SOLAR_COLUMN["general"] <= near_guard
    assert ode.SOLAR_TABLES["general"] <= near_guard
    # The conservative cut costs a layer no more than its criterion, k2*(1 + t*t) <= 1e-10; along
    # a column the levels' shares add up, the more the oftener light passes them (measured only).
    assert ode.SOLAR_LAYER["conservative"] <= ts.CONSERVATIVE


@pytest.mark.parametrize("linear", [False, True])
def test_thermal_mirror_against_the_equations_by_branch(linear):
    measured = thermal_measured()[linear]
    layer, column, tables = (ode.SOURCE_LAYER, ode.SOURCE_COLUMN, ode.SOURCE_TABLES) if linear \
        else (ode.THERMAL_LAYER, ode.THERMAL_COLUMN, ode.THERMAL_TABLES)
    title = "SOURCE" if linear else "THERMAL"
    check_recorded(title + "_LAYER", measured["layer"], layer)
    check_recorded(title + "_COLUMN", measured["column"], column)
    check_recorded(title + "_TABLES", measured["tables"], tables)
    # Neither has a quotient that cancels: rounding of the two long-double routes, level by level.
    for name in ("clear", "general"):
        assert layer[name] <= ode.REFERENCE_BOUND
        assert tables[name] <= (max(ode.DEPTHS) + 1)*ode.REFERENCE_BOUND
    assert layer["conservative"] <= tc.CONSERVATIVE


def test_conservative_em_stays_within_the_estimate_of_section_25():
    """em = (dif*t)/(1 + x) lacks the factor (1 + su*t/2) of the first-order limit: at most about
    k2*t*t/2 <= 5e-11 of piB."""
    worst, fraction, elements = thermal_measured()["em"]
    assert elements > 100
    print("conservative em: worst |em - reference| %.3g of piB, %.3g of k2*t*t/2" % (
        worst, fraction))
    assert fraction <= 1.
    recorded("EM_FRACTION", fraction, ode.EM_FRACTION)


# ---------------------------------------------------------------------------------------------
# The guard alone.
GUARD_TAU = (0.1, 0.5, 1., 3., 10.)
GUARD_OMEGA = (0.1, 0.4, 0.686, 0.75)
GUARD_G = (0., 0.47, 0.9)
# Both sides, the centre, the edges from inside and outside, and out to 2e-4.
GUARD_X = np.unique(np.concatenate([np.linspace(-2e-4, 2e-4, 41),
                                    [0.99e-4, -0.99e-4, 0.9999e-4, -0.9999e-4,
                                     1.0001e-4, -1.0001e-4]]))
# The Suns at which the scatterer is chosen for the Sun (the zenith among them, where the guard
# costs most), and the depths there: 41 from 0.1 to 10, which brackets the worst one within 6 %.
GUARD_MU0 = (1., 0.8, 0.6, 0.52)       # k2 = 4 at w = 0: no k*mu0 = 1 under mu0 = 1/2
GUARD_T = 10.**np.linspace(-1., 1., 41)
LAYER_KEYS = ("t", "w", "gp", "k2", "x", "branch", "above", "tau", "mu0")


def joined(parts):
    """Several layer_inputs as one, every array flat."""
    return {key: np.concatenate([np.ravel(part[key]) for part in parts]) for key in LAYER_KEYS}


def guard_scan():
    """layer_inputs of single layers at k*mu0 = 1 + GUARD_X, mu0 <= 1, and their g_c.  First the
    scatterer is given and the Sun follows, mu0 = (1 + x)/k, where that is at most 1.  Then the
    Sun is given, GUARD_MU0, and the scatterer follows: with a = 1 - w and c = 3*(1 - gp) the
    equations' k2 = 2*a*(c*(1 - a)/2 + 2*a) is (4 - c)*a*a + c*a, so a is the root of that
    quadratic at k2 = ((1 + x)/mu0)^2; omega_c = w/(1 - f + w*f) undoes the delta scaling, f = g*g,
    and tau_c = t/(1 - omega_c*f)."""
    tau, omega, g, x = (a.ravel() for a in np.meshgrid(GUARD_TAU, GUARD_OMEGA, GUARD_G, GUARD_X,
                                                       indexing="ij"))
    w_c = omega*tau
    table = np.stack([np.ones_like(tau), np.zeros_like(tau), tau, w_c, w_c*g], axis=1)
    k = np.sqrt(ts.layer_inputs(table, 1., np.zeros_like(tau), 0.)["k2"])
    mu0 = (1. + x)/k
    keep = mu0 <= 1.
    first = ts.layer_inputs(table[keep], mu0[keep], np.zeros(int(np.sum(keep))), 0.)
    t, sun, g2, x = (a.ravel() for a in np.meshgrid(GUARD_T, GUARD_MU0, (0., 0.5, 0.9), GUARD_X,
                                                    indexing="ij"))
    c = 3.*(1. - g2/(1. + g2))
    k2 = ((1. + x)/sun)**2
    a = (-c + np.sqrt(c*c + 4.*(4. - c)*k2))/(2.*(4. - c))
    w, f = 1. - a, g2*g2
    omega = w/(1. - f + w*f)
    tau = t/(1. - omega*f)
    assert np.all((omega > 0.) & (omega < 1.))
    w_c = omega*tau
    table = np.stack([np.ones_like(tau), np.zeros_like(tau), tau, w_c, w_c*g2], axis=1)
    second = ts.layer_inputs(table, sun, np.zeros_like(tau), 0.)
    # The float64 k*mu0 lands where it was asked for, far nearer than the 1e-8 that the points
    # next to the guard's edges keep from them.
    assert np.all(np.abs(second["x"] - (1. + x)) <= 1e-12)
    return joined([first, second]), np.concatenate([g[keep], g2])


def guard_table_elements():
    """layer_inputs of every element of two_stream_cases.resonance() and of the guard tables of
    the GPU tests, flat."""
    return joined([inputs.layer_inputs(False) for inputs in [ts.resonance()] + ode.guard_tables()])


def test_resonance_guard_costs_what_is_recorded_and_falls_to_zero_at_its_edges():
    """Inside the guard the layer is solved at mu0 = (1 +- 1e-4)/k in place of its own: the error
    of Rdir and Tdp is that of a shift of mu0 by (1e-4 - |1 - x|)/k, x = k*mu0, so it is bounded
    by a constant times 1e-4 - |1 - x|.  Outside, the general branch is exact up to rounding, which
    the quotient by (1 - x)*(1 + x) amplifies by up to 1e4: 64*2^-64/1e-4 = 3.5e-14 is allowed."""
    li, g = guard_scan()
    rounding = LD(64.*2.**-64/ode.GUARD)
    inside = li["branch"] == ts.GUARDED
    distance = (LD(ode.GUARD) - np.abs(LD(1.) - li["x"].astype(LD)))
    assert np.array_equal(inside, distance > 0.) and np.all(li["branch"][~inside] == ts.GENERAL)
    assert np.count_nonzero(inside & li["above"]) > 100
    assert np.count_nonzero(inside & ~li["above"]) > 100
    assert np.any(np.abs(1. - li["x"]) < 1e-9) and np.count_nonzero(~inside) > 100
    assert {0., 0.9} <= set(g[inside]) and np.all(li["mu0"] <= 1.) and np.any(li["mu0"] == 1.)
    mirror, reference = ts.layer(LD, li), ode.solar_layer(li)
    error = np.maximum(np.abs(mirror[2] - reference[2]), np.abs(mirror[3] - reference[3]))
    worst = int(np.argmax(error))
    print("guard: worst error of Rdir and Tdp %.4g of F0 at t = %.3g, w = %.3g, gp = %.3g, "
          "mu0 = %.4g, k*mu0 - 1 = %.3g" % (float(error[worst]), li["t"][worst], li["w"][worst],
                                            li["gp"][worst], li["mu0"][worst],
                                            li["x"][worst] - 1.))
    print("guard: worst error outside %.3g" % float(np.max(error[~inside])))
    assert np.all(error[~inside] <= rounding)
    # Rdif and Tdif do not know the Sun.
    assert np.all(np.abs(mirror[0] - reference[0]) <= ROUNDING)
    assert np.all(np.abs(mirror[1] - reference[1]) <= ROUNDING)
    deep = inside & (distance >= 1e-6)
    slope = float(np.max(error[deep]/distance[deep]))
    print("guard: worst error / (1e-4 - |1 - x|) %.4g" % slope)
    assert np.all(error[inside] <= LD(ode.GUARD_SLOPE)*distance[inside] + rounding)
    assert np.any(li["mu0"][inside] == 1.) and li["mu0"][worst] == 1.
    recorded("GUARD_ERROR", float(error[worst]), ode.GUARD_ERROR)
    recorded("GUARD_SLOPE", slope, ode.GUARD_SLOPE)
    # The same shape holds for every guarded element of the tables that run through the guard,
    # the mirror's own and the GPU tests', and the layer figure recorded for them obeys it.
    tables = guard_table_elements()
    inside = tables["branch"] == ts.GUARDED
    distance = (LD(ode.GUARD) - np.abs(LD(1.) - tables["x"].astype(LD)))
    mirror, reference = ts.layer(LD, tables), ode.solar_layer(tables)
    error = np.maximum(np.abs(mirror[2] - reference[2]), np.abs(mirror[3] - reference[3]))
    assert np.count_nonzero(inside) > 1000 and np.any(tables["mu0"][inside] == 1.)
    print("guard, tables: worst error %.4g, worst error / (1e-4 - |1 - x|) %.4g" % (
        float(np.max(error[inside])), float(np.max(error[inside]/distance[inside]))))
    assert np.all(error[inside] <= LD(ode.GUARD_SLOPE)*distance[inside] + rounding)
    assert np.all(error[inside] <= ode.GUARD_ERROR)
    assert ode.SOLAR_LAYER["guarded"] <= ode.GUARD_SLOPE*ode.GUARD + float(rounding)
    # The tables of the guard that the GPU test runs reach it on both sides and at the centre.
    for inputs in ode.guard_tables()[:3]:
        branch = inputs.layer_inputs(False)["branch"]
        assert np.all((branch == ts.GUARDED) == (np.abs(inputs.d) < ode.GUARD)[None, None, :])
        assert ode.guarded_elements(inputs) > 0


# ---------------------------------------------------------------------------------------------
# The tables of the GPU tests.
def test_tight_tables_have_no_element_in_the_guard():
    """Nothing is masked out in the GPU tests: the tables themselves keep out of the guard."""
    count = 0
    for inputs in ode.tight_solar_tables():
        for from_last in (False, True):
            count += ode.guarded_elements(inputs, from_last)
            assert not np.any(ode.solar_column_class(inputs.layer_inputs(from_last)) == 2)
    assert count == 0
    assert all(ode.guarded_elements(inputs) > 0 for inputs in ode.guard_tables())


def test_tables_reach_what_they_are_named_for():
    for columns, depth in ode.shapes():
        general = ode.solar_general(columns, depth)
        li = general.layer_inputs(False)
        assert np.all(ode.solar_column_class(li) == 0)
        assert np.any(li["branch"] == ts.IDENTITY) and np.any(li["w"] == 0.)
        if columns > 1:
            assert np.any(li["tau"] >= ode.LID)
        conservative = ode.solar_conservative(columns, depth)
        li = conservative.layer_inputs(False)
        exact = li["branch"][:, :, conservative.exact]
        assert np.all(exact == ts.CONSERVATIVE_BRANCH) and np.all(li["k2"][:, :, conservative.exact]
                                                                  == 0.)
        if columns > 1:
            near = li["w"][:, :, ~conservative.exact]
            assert np.all((near < 1.) & (near > 1. - 1e-10))
        thermal = ode.thermal_general(columns, depth)
        li = thermal.layer_inputs(False)
        assert set(ode.thermal_column_class(li).ravel()) <= {0, 1}
        assert np.any(li["tau"] == 0.) and (columns == 1 or np.any(li["tau"] >= ode.LID))
        li = ode.thermal_conservative(columns, depth).layer_inputs(False)
        assert np.any(li["k2"] == 0.) and np.all(li["branch"][li["k2"] == 0.] ==
                                                 tc.CONSERVATIVE_BRANCH)
    # Both sides of the conservative cut.
    for make, module in ((ode.solar_conservative, ts), (ode.thermal_conservative, tc)):
        branch = make(130, 17).layer_inputs(False)["branch"][:, :, 1::2]
        assert np.any(branch == module.CONSERVATIVE_BRANCH) and np.any(branch == module.GENERAL)
    # The spectral cases: at least three knots, and optics that differ within a level.
    for inputs in (ode.spectral_shortwave(), ode.spectral_longwave()):
        assert inputs.knots.size >= 3
        e = spectral.interpolate(inputs.knots, inputs.optics, inputs.nu)
        assert all(np.any(np.ptp(e[..., i], axis=1) > 0.) for i in range(3))


def test_float64_mirrors_keep_their_e_cpu_on_these_tables():
    """The GPU tests add 4*E_CPU of each entry's own case tables to their bounds: the float64
    mirror must not need more on the tables of this file."""
    for inputs, from_last in own_solar_tables():
        bound = spectral.E_CPU_SHORTWAVE if hasattr(inputs, "knots") else ts.E_CPU
        worst, finite = ts.worst_error(inputs, from_last)
        assert finite and worst <= bound, (inputs.name, worst)
    for inputs, from_last in own_thermal_tables():
        knots = hasattr(inputs, "knots")
        worst, finite = tc.worst_error(inputs.isothermal(), from_last)
        assert finite and worst <= (spectral.E_CPU_LONGWAVE if knots else tc.E_CPU), inputs.name
        worst, finite = tsc.worst_error(inputs, from_last)
        assert finite and worst <= (spectral.E_CPU_LONGWAVE if knots else tsc.E_CPU), inputs.name


# ---------------------------------------------------------------------------------------------
# The reference against 60 digits.
def exact(mp, value):
    """A long double as an mpf, bit for bit."""
    high = float(value)
    return mp.mpf(high) + mp.mpf(float(value - LD(high)))


def mp_operator(mp, matrix, t, growth, sources):
    """(R, T, up [sources], dn [sources]) from the matrix exponential of a whole layer, at enough
    digits for what cancels in it: exp(growth*t) squared."""
    with mp.workdps(70 + int(0.87*growth*t)):
        p = mp.expm(matrix*t, method="pade")
        r = -p[0, 1]/p[0, 0]
        tr = p[1, 0]*r + p[1, 1]
        up = [-p[0, 2 + i]/p[0, 0] for i in range(sources)]
        dn = [p[1, 0]*up[i] + p[1, 2 + i] for i in range(sources)]
        return +r, +tr, up, dn


def mp_solar(mp, t, w, gp, mu0):
    t, w, gp, mu0 = (mp.mpf(float(v)) for v in (t, w, gp, mu0))
    g2 = 3*w*(1 - gp)/4
    g1 = g2 + 2*(1 - w)
    g3 = (2 - 3*mu0*gp)/4
    matrix = mp.matrix([[g1, -g2, -w*g3/mu0], [g2, -g1, w*(1 - g3)/mu0], [0, 0, -1/mu0]])
    r, tr, up, dn = mp_operator(mp, matrix, t, g1 + g2, 1)
    return r, tr, up[0], dn[0], mp.exp(-t/mu0)


def mp_thermal(mp, t, w, gp, d):
    """(R, T, em, up1, dn1): the sources B = 1 and B = tau/t."""
    t, w, gp, d = (mp.mpf(float(v)) for v in (t, w, gp, d))
    g2 = d*w*(1 - gp)/2
    dif = d*(1 - w)
    g1 = g2 + dif
    # States I+, I-, 1 and tau/t, the source either the one or the other.
    one = mp.matrix([[g1, -g2, -dif, 0], [g2, -g1, dif, 0], [0, 0, 0, 0], [0, 0, 1/t, 0]])
    ramp = mp.matrix([[g1, -g2, 0, -dif], [g2, -g1, 0, dif], [0, 0, 0, 0], [0, 0, 1/t, 0]])
    r, tr, up, dn = mp_operator(mp, one, t, g1 + g2, 1)
    _, _, up1, dn1 = mp_operator(mp, ramp, t, g1 + g2, 1)
    return r, tr, up[0], up1[0], dn1[0]


SCAN_T = (1e-3, 0.03, 1., 30., 1e3)
SCAN_W = (0., 0.3, 0.9, 1. - 1e-6, 1.)
SCAN_GP = (0., 0.3, 0.47)
SCAN_MU0 = (1., 0.25, 1e-3)


def test_reference_against_sixty_digits():
    """Single layers by mp.expm over t from 1e-3 to 1e3, w from 0 to 1, gp to 0.47 and mu0 to
    1e-3, and 3-level columns by mp.lu_solve: the agreement is the reference's own rounding."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    t, w, gp, mu0 = (a.ravel() for a in np.meshgrid(SCAN_T, SCAN_W, SCAN_GP, SCAN_MU0,
                                                    indexing="ij"))
    solar = ode.solar_layer({"t": t, "w": w, "gp": gp, "mu0": mu0, "tau": t})
    worst = 0.
    for i in range(t.size):
        expect = mp_solar(mp, t[i], w[i], gp[i], mu0[i])
        worst = max(worst, max(float(abs(exact(mp, a[i]) - b)) for a, b in zip(solar, expect)))
    print("solar layers against 60 digits: worst %.3g" % worst)
    assert worst <= ode.REFERENCE_BOUND
    keep = mu0 == 1.
    t, w, gp = t[keep], w[keep], gp[keep]
    worst_thermal = 0.
    for d in (1.66, 2.):
        thermal = ode.thermal_layer({"t": t, "w": w, "gp": gp, "d": d})
        for i in range(t.size):
            expect = mp_thermal(mp, t[i], w[i], gp[i], d)
            worst_thermal = max(worst_thermal, max(float(abs(exact(mp, a[i]) - b))
                                                   for a, b in zip(thermal, expect)))
    print("thermal layers against 60 digits: worst %.3g" % worst_thermal)
    assert worst_thermal <= ode.REFERENCE_BOUND

    # Columns of three levels: the same equations between the interfaces, solved by LU.
    def mp_column(operators, reflectance, surface_source):
        levels = len(operators)
        n = 2*(levels + 1)
        a, b = mp.zeros(n, n), mp.zeros(n, 1)
        for i, (r, tr, s_up, s_dn) in enumerate(operators):
            a[2*i, i], a[2*i, levels + 1 + i], a[2*i, i + 1] = 1, -r, -tr
            a[2*i + 1, levels + 2 + i], a[2*i + 1, levels + 1 + i], a[2*i + 1, i + 1] = 1, -tr, -r
            b[2*i], b[2*i + 1] = s_up, s_dn
        a[n - 2, levels + 1] = 1
        a[n - 1, levels], a[n - 1, n - 1] = 1, -reflectance
        b[n - 1] = surface_source
        x = mp.lu_solve(a, b)
        return [x[i] for i in range(levels + 1)], [x[levels + 1 + i] for i in range(levels + 1)]

    worst_column = 0.
    layers = [(0.2, 0.95, 0.4), (30., 1. - 1e-6, 0.2), (1.5, 0.5, 0.)]
    for sun, albedo in ((1., 1.), (0.25, 0.3), (1e-3, 0.)):
        li = {name: np.array([layer[i] for layer in layers])[:, None]
              for i, name in enumerate(("t", "w", "gp"))}
        li["mu0"], li["tau"] = np.full((3, 1), sun), li["t"]
        got = ode.solar_column(ode.solar_layer(li), albedo, 1.)
        beam, operators = mp.mpf(1), []
        for layer in layers:
            r, tr, rdir, tdp, d = mp_solar(mp, *layer, sun)
            operators.append((r, tr, rdir*beam, tdp*beam))
            beam *= d
        up, diffuse = mp_column(operators, mp.mpf(albedo), mp.mpf(albedo)*beam)
        for i in range(4):
            worst_column = max(worst_column, float(abs(exact(mp, got["up"][i, 0]) - up[i])),
                               float(abs(exact(mp, got["diffuse"][i, 0]) - diffuse[i])))
    faces = np.array([0.3, 1., 0.6, 0.9])
    for eps in (1., 0.3, 0.):
        li = {name: np.array([layer[i] for layer in layers])[:, None]
              for i, name in enumerate(("t", "w", "gp"))}
        li["d"] = 1.66
        bt, bb = faces[:-1, None].astype(LD), faces[1:, None].astype(LD)
        got = ode.thermal_column(ode.thermal_layer(li), bt, bb, eps, LD(0.8))
        operators = []
        for i, layer in enumerate(layers):
            r, tr, em, up1, dn1 = mp_thermal(mp, *layer, 1.66)
            top, db = mp.mpf(float(faces[i])), mp.mpf(float(faces[i + 1])) - mp.mpf(float(faces[i]))
            operators.append((r, tr, top*em + db*up1, top*em + db*dn1))
        up, down = mp_column(operators, 1 - mp.mpf(eps), mp.mpf(eps)*mp.mpf(float(LD(0.8))))
        for i in range(4):
            worst_column = max(worst_column, float(abs(exact(mp, got["up"][i, 0]) - up[i])),
                               float(abs(exact(mp, got["down"][i, 0]) - down[i])))
    print("3-level columns against 60 digits: worst %.3g" % worst_column)
    # Four interfaces, each the sum of what the three layers and the surface send to it.
    assert worst_column <= 4.*ode.REFERENCE_BOUND
    recorded("REFERENCE_ERROR", max(worst, worst_thermal, worst_column/4.), ode.REFERENCE_ERROR)
