"""CPU-only checks of the five view products against the transfer equation itself
(tests/radiance_ode_cases.py: a long-double solver that carries pi*I along either ray as one more
state of two_stream_ode_cases' linear system and knows none of the closed forms of the view):

(a) that solver against 60-digit mpmath, level by level and on 3-level columns;
(b) the long-double mirror chain -- the flux mirror feeding the view mirror -- against it, over the
    tables of the GPU tests at every depth, column count and order, the whole view and every
    observer in both directions, by product and by the class of the column;
(c) the gain of the view mirrors with respect to one flux row;
(d) that the tables hold what the GPU tests rely on, so that nothing is masked there;
(e) that the comparison of (b) has teeth: two deliberately wrong references fail it.

Every measured figure is printed, and recorded as a constant of tests/radiance_ode_cases.py that
must satisfy measured <= CONSTANT <= 2*measured."""
import functools

import numpy as np
import pytest

from tests import radiance_ode_cases as rad
from tests import solar_radiance_cases as svc
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_radiance_observer_cases as oc
from tests import two_stream_cases as ts
from tests import two_stream_ode_cases as ode

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
MU = rad.MU
THERMAL_FLUXES, SOLAR_FLUXES = ("up", "down"), ("up", "direct", "diffuse")


def recorded(what, measured, constant):
    """The 2x rule of a constant that records a measured figure."""
    print("%s: measured %.3g, recorded %.3g" % (what, measured, constant))
    assert measured <= constant <= 2.*measured, \
        "radiance_ode_cases: %s no longer records the measured %.3g" % (what, measured)


def relative(error, scale):
    """error/scale where scale > 0; where it is 0 the two must agree exactly."""
    assert np.all(np.isfinite(error))
    dark = scale == 0.
    assert np.all(error[dark] == 0.)
    return np.where(dark, 0., error/np.where(dark, 1., scale))


def thermal_tables():
    return [(name, columns, depth) for name in rad.THERMAL_MAKERS for columns, depth in
            ode.shapes()] + [("spectral",) + ode.SPECTRAL_SHAPE[:2]]


def solar_tables():
    return [(name, columns, depth) for name in rad.SOLAR_MAKERS for columns, depth in
            ode.shapes()] + [("spectral",) + ode.SPECTRAL_SHAPE[:2]]


def thermal_sweeps(problem, from_last, fluxes):
    return rad.thermal_mirror_sweeps(problem, MU, from_last, fluxes)


def thermal_chain(name, columns, depth, from_last, linear):
    """(|chain - reference|/scale [PATHS, columns], worst over the whole view and every
    observer in both directions; the layer inputs)."""
    inputs, reference = rad.thermal_case(name, columns, depth, from_last)
    reference = reference[linear]
    problem = rad.thermal_problem(inputs, linear)
    fluxes = rad.rows(rad.thermal_flux_mirror(inputs, from_last, linear), THERMAL_FLUXES)
    whole = rad.whole_view_mirror(inputs, MU, from_last, linear, fluxes)
    error = relative(np.abs(whole - reference["down"][0]), reference["scale"])
    if not rad.spectral(inputs):
        sweeps = thermal_sweeps(problem, from_last, fluxes)
        assert np.array_equal(sweeps[False][0], whole)
        for up in (False, True):
            for n in rad.observers(depth):
                got = rad.at_observer(sweeps[up], n, up)
                want = rad.at_observer(reference["up" if up else "down"], n, up)
                error = np.maximum(error, relative(np.abs(got - want), reference["scale"]))
    return error, inputs.layer_inputs(from_last)


def solar_chain(name, columns, depth, from_last):
    inputs, cosine, reference = rad.solar_case(name, columns, depth, from_last)
    fluxes = rad.rows(rad.solar_flux_mirror(inputs, from_last), SOLAR_FLUXES)
    high = rad.solar_view_mirror(inputs, MU, cosine, from_last, fluxes)
    scale = svc.scale(inputs, high)
    return relative(np.abs(high["radiance"] - reference["down"][0]), scale), \
        inputs.layer_inputs(from_last)


@functools.lru_cache(maxsize=None)
def chain_measured():
    out = {product: dict.fromkeys(rad.CHAIN[product], 0.) for product in rad.PRODUCTS}
    for name, columns, depth in thermal_tables():
        for from_last in (False, True):
            for linear in ((False,) if name == "spectral" else (False, True)):
                error, li = thermal_chain(name, columns, depth, from_last, linear)
                into = out["linear" if linear else "isothermal"]
                classes = ode.thermal_column_class(li)
                for index, label in enumerate(ode.THERMAL_CLASSES):
                    into[label] = max(into[label], float(np.max(error[classes == index],
                                                                initial=0.)))
    for name, columns, depth in solar_tables():
        for from_last in (False, True):
            error, li = solar_chain(name, columns, depth, from_last)
            classes = ode.solar_column_class(li)
            for index, label in enumerate(ode.SOLAR_CLASSES):
                out["solar"][label] = max(out["solar"][label],
                                          float(np.max(error[classes == index], initial=0.)))
    return out


@pytest.mark.parametrize("product", rad.PRODUCTS)
def test_mirror_chain_against_the_transfer_equation_by_class(product):
    """Where every level is general, clear or exactly conservative the chain differs from the
    equations by the float64 rounding of its flux rows times the view's gain and no more; the
    conservative cut and the guard cost what is recorded."""
    measured = chain_measured()[product]
    for label in rad.CHAIN[product]:
        recorded("CHAIN[%s][%s]" % (product, label), measured[label], rad.CHAIN[product][label])
    # Clear: every flux row is rounded to float64 once (2^-53 of its own size, at most the flux
    # scale), two or three rows enter a level, and a ray passes up to 17 levels.
    if "clear" in rad.CHAIN[product]:
        assert rad.CHAIN[product]["clear"] <= 3.*max(ode.DEPTHS)*rad.GAIN[product]*2.**-53
    # General: that, and the mirror's own long-double rounding where its quotients amplify it:
    # by 1/n >= 1e5 just above the conservative threshold (k*sqrt(1 + t*t) > 1e-5 there and n is
    # about 2*k*(1/g2 + t)), with the linear source times the shift c <= 1/(su*t) <= 1e3 of pi*dB
    # (t >= 1e-3 in these tables); by 1/GUARD next to the guard, as two_stream_ode_cases allows.
    amplified = {"isothermal": 1e5, "linear": 1e8, "solar": 1./ode.GUARD}[product]
    assert rad.CHAIN[product]["general"] <= 3.*max(ode.DEPTHS)*rad.GAIN[product]*2.**-53 + \
        amplified*ode.REFERENCE_BOUND
    # The conservative cut and the guard are recorded as measured, as two_stream_ode_cases'
    # *_TABLES are: a level's share adds up along the column.


# ---------------------------------------------------------------------------------------------
# (c) The gain of the view with respect to its flux rows.
def perturbed(fluxes, q, level, delta):
    out = dict(fluxes)
    out[q] = fluxes[q].copy()
    out[q][level] += delta
    return out


@functools.lru_cache(maxsize=None)
def gain_measured():
    """{product: the largest |change of the long-double view mirror|/scale per |change of one flux
    row|/(flux scale)}: one row (every column of one flat level) moved by 2^-10 of the flux scale
    at a time, every view of (b) read."""
    out = dict.fromkeys(rad.PRODUCTS, 0.)
    step = LD(2.)**-10
    pi = LD(cases.FLUX_PI)
    for name, columns, depth in thermal_tables():
        for from_last in (False, True):
            inputs, reference = rad.thermal_case(name, columns, depth, from_last)
            if name == "spectral":                                  # the whole view alone
                scale = reference[False]["scale"]
                flux_scale = (pi*scale).astype(F64)
                fluxes = rad.rows(rad.thermal_flux_mirror(inputs, from_last, False),
                                  THERMAL_FLUXES)
                base = rad.whole_view_mirror(inputs, MU, from_last, False, fluxes)
                for level in range(inputs.levels):
                    delta = (step*flux_scale[level//depth]).astype(F64)
                    for q in THERMAL_FLUXES:
                        moved = rad.whole_view_mirror(inputs, MU, from_last, False,
                                                      perturbed(fluxes, q, level, delta))
                        out["isothermal"] = max(out["isothermal"], float(np.max(
                            relative(np.abs(moved - base), scale))/step))
                continue
            for linear in (False, True):
                problem = rad.thermal_problem(inputs, linear)
                scale = reference[linear]["scale"]
                lit = scale > 0.
                flux_scale = (pi*scale).astype(F64)                 # [PATHS, columns]
                fluxes = rad.rows(rad.thermal_flux_mirror(inputs, from_last, linear),
                                  THERMAL_FLUXES)
                base = thermal_sweeps(problem, from_last, fluxes)
                worst = 0.
                for level in range(inputs.levels):
                    delta = (step*flux_scale[level//depth]).astype(F64)
                    for q in THERMAL_FLUXES:
                        moved = thermal_sweeps(problem, from_last,
                                               perturbed(fluxes, q, level, delta))
                        for up in (False, True):
                            change = np.abs(moved[up] - base[up])[:, lit]/scale[lit]
                            worst = max(worst, float(np.max(change, initial=0.)/step))
                product = "linear" if linear else "isothermal"
                out[product] = max(out[product], worst)
    for name, columns, depth in solar_tables():
        for from_last in (False, True):
            inputs, cosine, _ = rad.solar_case(name, columns, depth, from_last)
            fluxes = rad.rows(rad.solar_flux_mirror(inputs, from_last), SOLAR_FLUXES)
            base = rad.solar_view_mirror(inputs, MU, cosine, from_last, fluxes)
            scale = svc.scale(inputs, base)
            f0 = inputs.f0()
            for level in range(inputs.levels):
                delta = (step*f0[level//depth]).astype(F64)
                for q in SOLAR_FLUXES:
                    moved = rad.solar_view_mirror(inputs, MU, cosine, from_last,
                                                  perturbed(fluxes, q, level, delta))
                    change = relative(np.abs(moved["radiance"] - base["radiance"]), scale)
                    out["solar"] = max(out["solar"], float(np.max(change)/step))
    return out


def test_gain_of_the_view_with_respect_to_one_flux_row():
    """From the mirrors alone.  A unit of flux scale in one row is pi*scale of the longwave
    views, which read it through (w/(2 pi))*(1 + a) and a weight below 1: the gain stays near 1."""
    measured = gain_measured()
    for product in rad.PRODUCTS:
        recorded("GAIN[%s]" % product, measured[product], rad.GAIN[product])


# ---------------------------------------------------------------------------------------------
# (d) The tables.
def test_tables_hold_what_the_gpu_tests_rely_on():
    signs = {True: 0, False: 0}
    for columns, depth in ode.shapes():
        for from_last in (False, True):
            general = ode.thermal_general(columns, depth)
            li = general.layer_inputs(from_last)
            assert set(ode.thermal_column_class(li).ravel()) <= {0, 1}
            assert np.any(li["branch"] == tc.CLEAR) and np.any(li["tau"] == 0.)
            assert columns == 1 or np.any(li["tau"] >= ode.LID)
            cloudy = (li["branch"] != tc.CLEAR) & (li["tau"] > 0.)
            positive, _, _ = rc.decisions(li, MU[None, :, None])
            positive = np.broadcast_to(positive, cloudy.shape)
            if depth >= 9:
                assert np.any(positive[cloudy]) and np.any(~positive[cloudy]), (columns, depth)
            signs[True] += int(np.count_nonzero(positive[cloudy]))
            signs[False] += int(np.count_nonzero(~positive[cloudy]))
            # An observer strictly inside a cloud: cloudy levels on both sides of its interface.
            inside = 0
            for n in rad.observers(depth):
                if 0 < n < depth:
                    inside += int(np.count_nonzero(cloudy[n - 1] & cloudy[n])) + \
                        int(np.count_nonzero(cloudy[depth - n - 1] & cloudy[depth - n]))
            if depth >= 2:
                assert inside > 0, (columns, depth)
            solar = ode.solar_general(columns, depth)
            li = solar.layer_inputs(from_last)
            assert np.all(ode.solar_column_class(li) == 0)
            vi = svc.problem_inputs(solar, from_last)
            assert np.any(vi["branch"] == ts.IDENTITY) and np.any(vi["branch"] == svc.NO_SCATTERING)
            assert columns == 1 or np.any(li["tau"] >= ode.LID)
            scattering = ~np.isin(vi["branch"], (ts.IDENTITY, svc.NO_SCATTERING))
            positive, _ = svc.decisions(vi, MU[None, :, None])
            positive = np.broadcast_to(positive, scattering.shape)
            if depth >= 9:
                assert np.any(positive[scattering]) and np.any(~positive[scattering])
            for make in (ode.solar_general, ode.solar_conservative):
                assert ode.guarded_elements(make(columns, depth), from_last) == 0
            assert ode.guarded_elements(ode.solar_guard(columns, depth), from_last) > 0
    assert signs[True] > 1000 and signs[False] > 1000
    for inputs in (ode.spectral_shortwave(), ode.spectral_longwave()):
        assert inputs.knots.size >= 3
    assert ode.guarded_elements(ode.spectral_shortwave()) == 0
    assert rad.observers(1) == [0, 1] and rad.observers(2) == [0, 1, 2]
    assert rad.observers(17) == [0, 1, 16, 17]


# ---------------------------------------------------------------------------------------------
# (e) Two wrong references.
def general_deviation():
    worst = 0.
    for from_last in (False, True):
        inputs = ode.thermal_general(64, 9)
        reference = rad.thermal_reference(inputs, MU, from_last)
        for linear in (False, True):
            problem = rad.thermal_problem(inputs, linear)
            fluxes = rad.rows(rad.thermal_flux_mirror(inputs, from_last, linear), THERMAL_FLUXES)
            sweeps = thermal_sweeps(problem, from_last, fluxes)
            for up in (False, True):
                want = reference[linear]["up" if up else "down"]
                got = sweeps[up]
                worst = max(worst, float(np.max(relative(
                    np.abs(got - want), np.broadcast_to(reference[linear]["scale"], got.shape)))))
    return worst


def test_a_wrong_reference_is_caught(monkeypatch):
    """The comparison of (b) fails by orders of magnitude for a reference whose downward ray has
    `a` with the upward ray's sign, and for one whose rays read interface i in place of i + 1 for
    the flux entering a level from below."""
    bound = rad.CHAIN["isothermal"]["general"]
    assert general_deviation() <= max(rad.CHAIN["isothermal"]["general"],
                                      rad.CHAIN["linear"]["general"])
    honest_rows = rad._ray_rows

    def same_sign(m, mu, w, a, source_columns, source):
        honest_rows(m, mu, w, a, source_columns, source)
        d = m.shape[-1] - 1
        m[..., d, 0], m[..., d, 1] = m[..., d, 1].copy(), m[..., d, 0].copy()
    monkeypatch.setattr(rad, "_ray_rows", same_sign)
    wrong = general_deviation()
    print("downward ray with the upward ray's a: %.3g of scale" % wrong)
    assert wrong > 1e6*bound
    monkeypatch.setattr(rad, "_ray_rows", honest_rows)
    honest_rays = rad.rays

    def shifted(view, up, down, source_up, source_down, start):
        return honest_rays(view, np.concatenate([up[:1], up[:-1]]), down, source_up, source_down,
                           start)
    monkeypatch.setattr(rad, "rays", shifted)
    wrong = general_deviation()
    print("interface i in place of i + 1: %.3g of scale" % wrong)
    assert wrong > 1e6*bound


# ---------------------------------------------------------------------------------------------
# (a) The reference against 60 digits.
def exact(mp, value):
    """A long double as an mpf, bit for bit."""
    high = float(value)
    return mp.mpf(high) + mp.mpf(float(value - LD(high)))


VIEW_KEYS = ("rt", "td", "up", "dn", "ut", "u_dn", "u_up", "u_src", "dt", "d_dn", "d_up", "d_src")


def mp_view(mp, matrix, t, growth, sources):
    """The View of one level as a dict of VIEW_KEYS from the matrix exponential of the whole
    augmented system (states I+, I-, the source states, U, D), at enough digits for what cancels
    in it: exp(growth*t) squared."""
    n = matrix.rows
    u, d = n - 2, n - 1
    with mp.workdps(70 + int(0.87*growth*t)):
        p = mp.expm(matrix*t, method="pade")
        tu = 1/p[0, 0]
        r = -p[0, 1]*tu
        up = [-p[0, 2 + i]*tu for i in range(sources)]
        ut = 1/p[u, u]
        out = {"rt": r, "td": p[1, 0]*r + p[1, 1], "up": up,
               "dn": [p[1, 0]*up[i] + p[1, 2 + i] for i in range(sources)],
               "ut": ut, "u_dn": -(p[u, 0]*r + p[u, 1])*ut, "u_up": -(p[u, 0]*tu)*ut,
               "u_src": [-(p[u, 0]*up[i] + p[u, 2 + i])*ut for i in range(sources)],
               "dt": p[d, d], "d_dn": p[d, 0]*r + p[d, 1], "d_up": p[d, 0]*tu,
               "d_src": [p[d, 0]*up[i] + p[d, 2 + i] for i in range(sources)]}
        return {key: ([+x for x in value] if isinstance(value, list) else +value)
                for key, value in out.items()}


def mp_on_top(a, b):
    """Two levels as one, at 60 digits: the two flux relations of either level solved for the
    fluxes between them, and each ray through one level after the other.  (Both levels are
    symmetric: rb = rt and tu = td.)"""
    m = 1/(1 - a["rt"]*b["rt"])
    count = range(len(a["up"]))
    dn_t, dn_b = a["td"]*m, a["rt"]*b["td"]*m
    dn_s = [(a["dn"][i] + a["rt"]*b["up"][i])*m for i in count]
    up_t, up_b = b["rt"]*a["td"]*m, b["td"]*m
    up_s = [(b["up"][i] + b["rt"]*a["dn"][i])*m for i in count]
    return {"rt": a["rt"] + a["td"]*up_t, "td": b["td"]*dn_t,
            "up": [a["up"][i] + a["td"]*up_s[i] for i in count],
            "dn": [b["dn"][i] + b["td"]*dn_s[i] for i in count],
            "ut": a["ut"]*b["ut"],
            "u_dn": a["u_dn"] + a["u_up"]*up_t + a["ut"]*b["u_dn"]*dn_t,
            "u_up": a["u_up"]*up_b + a["ut"]*(b["u_up"] + b["u_dn"]*dn_b),
            "u_src": [a["u_src"][i] + a["u_up"]*up_s[i] + a["ut"]*(b["u_src"][i] +
                                                                   b["u_dn"]*dn_s[i])
                      for i in count],
            "dt": a["dt"]*b["dt"],
            "d_dn": b["d_dn"]*dn_t + b["dt"]*(a["d_dn"] + a["d_up"]*up_t),
            "d_up": b["d_up"] + b["d_dn"]*dn_b + b["dt"]*a["d_up"]*up_b,
            "d_src": [b["d_src"][i] + b["d_dn"]*dn_s[i] + b["dt"]*(a["d_src"][i] +
                                                                   a["d_up"]*up_s[i])
                      for i in count]}


MP_WHOLE = 40.      # growth*t up to which one matrix exponential takes the whole level


def mp_level(mp, matrix, t, growth, sources, lower):
    """mp_view of a level of any thickness: the whole level by one matrix exponential where
    growth*t <= MP_WHOLE; beyond, 2^n equal parts of it by theirs, put on top of each other at 60
    digits (the matrix exponential of t/mu = 20 000 would take 17 000 digits)."""
    n = 0
    while growth*t/2**n > MP_WHOLE:
        n += 1
    h = t/2**n
    view = mp_view(mp, matrix, h, growth, sources)
    for j in range(n):
        below = dict(view)
        for key in ("up", "dn", "u_src", "d_src"):
            below[key] = lower(view[key], h*2**j)
        view = mp_on_top(view, below)
    return view


def mp_thermal_matrix(mp, w, gp, d, mu):
    g2 = d*w*(1 - gp)/2
    dif = d*(1 - w)
    g1 = g2 + dif
    a = 3*gp*mu/2
    forth, back, source = (w/2)*(1 + a)/mu, (w/2)*(1 - a)/mu, (1 - w)/mu
    return mp.matrix([[g1, -g2, -dif, 0, -dif, 0, 0], [g2, -g1, dif, 0, dif, 0, 0],
                      [0]*7, [0]*7, [0, 0, 0, 1, 0, 0, 0],
                      [-forth, -back, -source, 0, -source, 1/mu, 0],
                      [back, forth, source, 0, source, 0, -1/mu]]), g1 + g2 + 1/mu


def mp_thermal(mp, t, w, gp, d, mu):
    """The level under pi*B = 1 (source 0) and pi*B = tau/t (source 1)."""
    t, w, gp, d, mu = (mp.mpf(float(v)) for v in (t, w, gp, d, mu))
    matrix, growth = mp_thermal_matrix(mp, w, gp, d, mu)
    view = mp_level(mp, matrix, t, growth, 2, lambda s, depth: [s[0], depth*s[0] + s[1]])
    for key in ("up", "dn", "u_src", "d_src"):
        view[key] = [view[key][0], view[key][1]/t]
    return view


SOLAR_SCATTERER = dict(osc=0.8, tau_r=0.5, w_c=1., tau_s=1.5, gc=0.5)
COS_THETA = -0.3


def mp_solar(mp, t, w, gp, mu0, mu):
    t, w, gp, mu0, mu = (mp.mpf(float(v)) for v in (t, w, gp, mu0, mu))
    osc, tau_r, w_c, tau_s, gc = (mp.mpf(SOLAR_SCATTERER[name]) for name in
                                  ("osc", "tau_r", "w_c", "tau_s", "gc"))
    c = mp.mpf(COS_THETA)
    pmix = (tau_r*3*(1 + c*c)/4 + w_c*(1 - gc*gc)/(1 + gc*gc - 2*gc*c)**mp.mpf(1.5))/tau_s
    g2 = 3*w*(1 - gp)/4
    g1 = g2 + 2*(1 - w)
    g3 = (2 - 3*mu0*gp)/4
    a = 3*gp*mu/2
    forth, back, source = (w/2)*(1 + a)/mu, (w/2)*(1 - a)/mu, (osc*pmix/4)/mu0/mu
    matrix = mp.matrix([[g1, -g2, -w*g3/mu0, 0, 0], [g2, -g1, w*(1 - g3)/mu0, 0, 0],
                        [0, 0, -1/mu0, 0, 0], [-forth, -back, -source, 1/mu, 0],
                        [back, forth, source, 0, -1/mu]])
    return mp_level(mp, matrix, t, g1 + g2 + 1/mu, 1,
                    lambda s, depth: [mp.exp(-depth/mu0)*x for x in s])


def view_parts(view, index):
    """VIEW_KEYS of element `index` of a radiance_ode_cases.View (sources as lists)."""
    f = view.flux
    parts = {"rt": f.rt, "td": f.td, "up": f.up, "dn": f.dn}
    parts.update(zip(rad.View.NAMES, view.parts()))
    parts.update(ut=view.ut, dt=view.dt)
    return {key: ([x[index] for x in value] if key in ("up", "dn", "u_src", "d_src")
                  else value[index]) for key, value in parts.items() if key in VIEW_KEYS}


def worst_difference(mp, got, expect, source_size=1.):
    """The worst |reference - 60 digits| over VIEW_KEYS; what a unit source sends into a ray in
    units of source_size, the size of that source's term of pi*J."""
    worst = 0.
    for key in VIEW_KEYS:
        pairs = zip(got[key], expect[key]) if isinstance(expect[key], list) else \
            [(got[key], expect[key])]
        size = source_size if key in ("u_src", "d_src") else 1.
        worst = max([worst] + [float(abs(exact(mp, a) - b))/size for a, b in pairs])
    return worst


def mp_quadrature(mp, matrix, t, mu, view, sources):
    """u_dn, d_dn, u_src[0] and d_src[0] of a level by direct quadrature of the transfer integral
        U(0) = int_0^t J+(tau) exp(-tau/mu) dtau/mu ; D(t) = int_0^t J-(tau) exp(-(t - tau)/mu) dtau/mu
    over the fluxes inside the level, y(tau) = exp(A tau) y(0) with y(0) from the level's own flux
    operator; against `view`.  The worst difference."""
    n = matrix.rows - 2
    block = matrix[:n, :n]
    worst = mp.mpf(0)
    starts = [("u_dn", "d_dn", [view["rt"], 1] + [0]*(n - 2))]
    first = [view["up"][0], 0] + [0]*(n - 2)
    first[2] = 1
    starts.append((("u_src", 0), ("d_src", 0), first))
    for key_up, key_down, start in starts:
        y0 = mp.matrix(start)

        def source(row, tau):
            y = mp.expm(block*tau, method="pade")*y0
            return -sum(matrix[row, j]*y[j] for j in range(n))*mu     # pi*J of the ray `row`
        upward = mp.quad(lambda tau: source(n, tau)*mp.exp(-tau/mu)/mu, [0, t])
        downward = mp.quad(lambda tau: -source(n + 1, tau)*mp.exp(-(t - tau)/mu)/mu, [0, t])
        for key, value in ((key_up, upward), (key_down, downward)):
            have = view[key[0]][key[1]] if isinstance(key, tuple) else view[key]
            worst = max(worst, abs(have - value))
    return float(worst)


SCAN_T = (1e-3, 0.03, 1., 30., 1e3)
SCAN_W = (0., 0.6, 1. - 1e-6, 1.)
SCAN_GP = (0., 0.47)
SCAN_MU0 = (1., 0.25, 1e-3)


def test_reference_against_sixty_digits():
    """Single levels over t from 1e-3 to 1e3, w from 0 to 1, gp to 0.47 at mu = 1, 0.6 and 0.05
    (the Sun at 1, 0.25 and 1e-3 in turn), every source and both rays, and 3-level columns: the
    agreement is the reference's own rounding.  Up to t = 1 the 60-digit side is itself held to
    the direct quadrature of the transfer integral."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    t, w, gp, mu = (a.ravel() for a in np.meshgrid(SCAN_T, SCAN_W, SCAN_GP, MU, indexing="ij"))
    mu0 = np.array(SCAN_MU0)[np.arange(t.size) % 3]
    view, thickness = rad.thermal_view({"t": t, "w": w, "gp": gp, "d": 1.66}, mu)
    safe = np.where(thickness > 0., thickness, 1.)
    for part in (view.flux.up, view.flux.dn, view.u_src, view.d_src):
        part[1] = part[1]/safe
    vi = {"t": t, "w": w, "gp": gp, "mu0": mu0, "tau": t}
    vi.update({name: np.full(t.shape, value) for name, value in SOLAR_SCATTERER.items()})
    solar, _, _ = rad.solar_view(vi, mu, np.full(t.shape, COS_THETA))
    beam_term = (SOLAR_SCATTERER["osc"]*rad.phase(vi, COS_THETA)/4./mu0).astype(F64)
    worst_thermal = worst_solar = worst_quadrature = 0.
    for i in range(t.size):
        expect = mp_thermal(mp, t[i], w[i], gp[i], 1.66, mu[i])
        worst_thermal = max(worst_thermal, worst_difference(mp, view_parts(view, i), expect))
        if t[i] <= 1. and w[i] == 0.6 and gp[i] > 0.:
            matrix, _ = mp_thermal_matrix(mp, mp.mpf(float(w[i])), mp.mpf(float(gp[i])),
                                          mp.mpf(1.66), mp.mpf(float(mu[i])))
            whole = mp_view(mp, matrix, mp.mpf(float(t[i])), 30., 2)
            worst_quadrature = max(worst_quadrature, mp_quadrature(
                mp, matrix, mp.mpf(float(t[i])), mp.mpf(float(mu[i])), whole, 2))
        expect = mp_solar(mp, t[i], w[i], gp[i], mu0[i], mu[i])
        # The beam's term of pi*J is ((omega/sc)*Pmix/4)/mu0 per unit of direct flux: 2e2 under
        # mu0 = 1e-3.
        worst_solar = max(worst_solar, worst_difference(mp, view_parts(solar, i), expect,
                                                        max(1., beam_term[i])))
    print("thermal levels against 60 digits: worst %.3g" % worst_thermal)
    print("solar levels against 60 digits: worst %.3g" % worst_solar)
    print("60-digit levels against the quadrature of the transfer integral: worst %.3g"
          % worst_quadrature)
    assert worst_quadrature <= 1e-45
    assert worst_thermal <= rad.REFERENCE_BOUND and worst_solar <= rad.REFERENCE_BOUND

    # Columns of three levels: the interface fluxes by LU, each ray level by level.
    def mp_column(levels, up_source, down_source, reflectance, surface_source):
        count = len(levels)
        n = 2*(count + 1)
        a, b = mp.zeros(n, n), mp.zeros(n, 1)
        for i, level in enumerate(levels):
            a[2*i, i], a[2*i, count + 1 + i], a[2*i, i + 1] = 1, -level["rt"], -level["td"]
            a[2*i + 1, count + 2 + i], a[2*i + 1, count + 1 + i], a[2*i + 1, i + 1] = \
                1, -level["td"], -level["rt"]
            b[2*i], b[2*i + 1] = up_source[i][0], down_source[i][0]
        a[n - 2, count + 1] = 1
        a[n - 1, count], a[n - 1, n - 1] = 1, -reflectance
        b[n - 1] = surface_source
        x = mp.lu_solve(a, b)
        up, down = [x[i] for i in range(count + 1)], [x[count + 1 + i] for i in range(count + 1)]
        looking_down = [0]*count + [surface_source + reflectance*down[count]]
        looking_up = [0]*(count + 1)
        for i in range(count - 1, -1, -1):
            looking_down[i] = levels[i]["ut"]*looking_down[i + 1] + levels[i]["u_dn"]*down[i] + \
                levels[i]["u_up"]*up[i + 1] + up_source[i][1]
        for i in range(count):
            looking_up[i + 1] = levels[i]["dt"]*looking_up[i] + levels[i]["d_dn"]*down[i] + \
                levels[i]["d_up"]*up[i + 1] + down_source[i][1]
        return looking_down, looking_up

    worst_column = 0.
    layers = [(0.2, 0.95, 0.4), (30., 1. - 1e-6, 0.2), (1.5, 0.5, 0.)]
    faces = np.array([0.3, 1., 0.6, 0.9])
    li = {name: np.array([layer[i] for layer in layers])[:, None]
          for i, name in enumerate(("t", "w", "gp"))}
    li["d"] = 1.66
    for view_mu, eps in ((1., 1.), (0.6, 0.3), (0.05, 0.)):
        view, thickness = rad.thermal_view(li, view_mu)
        f = view.flux
        bt, bb = faces[:-1, None].astype(LD), faces[1:, None].astype(LD)
        db = bb - bt
        flux = ode.thermal_column((f.rt, f.td, f.up[0], f.up[1]/thickness, f.dn[1]/thickness),
                                  bt, bb, eps, LD(0.8))
        start = LD(eps)*LD(0.8) + (LD(1.) - LD(eps))*flux["down"][-1]
        got = rad.rays(view, flux["up"], flux["down"],
                       bt*view.u_src[0] + db*view.u_src[1]/thickness,
                       bt*view.d_src[0] + db*view.d_src[1]/thickness, start)
        levels = [mp_thermal(mp, *layer, 1.66, view_mu) for layer in layers]
        top = [mp.mpf(float(x)) for x in faces[:-1]]
        step = [mp.mpf(float(faces[i + 1])) - mp.mpf(float(faces[i])) for i in range(3)]
        expect = mp_column(
            levels,
            [(top[i]*v["up"][0] + step[i]*v["up"][1], top[i]*v["u_src"][0] + step[i]*v["u_src"][1])
             for i, v in enumerate(levels)],
            [(top[i]*v["dn"][0] + step[i]*v["dn"][1], top[i]*v["d_src"][0] + step[i]*v["d_src"][1])
             for i, v in enumerate(levels)],
            1 - mp.mpf(eps), mp.mpf(eps)*mp.mpf(float(LD(0.8))))
        for ray in range(2):
            for i in range(4):
                worst_column = max(worst_column,
                                   float(abs(exact(mp, got[ray][i, 0]) - expect[ray][i])))
    print("3-level columns against 60 digits: worst %.3g" % worst_column)
    # Four interfaces, each the sum of what the three levels and the surface send to it.
    assert worst_column <= 4.*rad.REFERENCE_BOUND
    recorded("REFERENCE_ERROR", max(worst_thermal, worst_solar, worst_column/4.),
             rad.REFERENCE_ERROR)
