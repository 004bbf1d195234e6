"""What tests/test_solar_radiance_host.py (CPU), tests/test_gpu_solar_radiance_shapes.py and
tests/test_gpu_solar_radiance.py (GPU) share: the definition of
Spectroscopy.compute_solar_radiance in numpy -- the level of csrc/solar_radiance.h, for any float
type: float64 "as written", numpy.longdouble as the reference -- and the case tables.  The
problems and the two-stream fluxes are tests/two_stream_cases.py's.

Like two_stream_cases' mirror this one continues from the float64 layer inputs (t, w, gp, omega/sc,
tau_R, tau_s, w_c, gc) and the float64 branch decisions: identity, no scattering, conservative,
general or guarded and the guard's side, the side of y = 0 and the branch of linear_weight.  The
flux rows are inputs of the kernel: both float types read the same float64 rows, the float64
mirror of two_stream_cases.

scale[p, j] = max(F0/pi, the long-double mirror's largest |I| at the path's interfaces).

E_CPU is the worst |float64 mirror - long-double mirror|/scale over every case table of this file,
as tests/test_solar_radiance_host.py measures it; the GPU tests hold every radiance to
(4*E_CPU + FLOOR)*scale of the long-double mirror."""
import numpy as np

from tests import sweep_cases as cases
from tests import thermal_radiance_cases as rc
from tests import two_stream_cases as ts

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
VIEW_AHEAD = 1              # kSolarViewAhead
MU = (1., 0.6, 0.05)
MU0 = (1., 0.5, 0.1)
PHI = (0., 90., 180.)
# The worst error of the float64 mirror over the case tables, relative to scale (see above):
# tests/test_solar_radiance_host.py measures 7.9e-12, in two_stream_cases' shape tables.
E_CPU = 8e-12
E_CPU_CAP = 1e-10
FLOOR = 1e-13
# Bounds of the mirror's properties (tests/test_solar_radiance_host.py), each beside what was
# measured there.
QUADRATURE_BOUND = 5e-17    # |closed form - quadrature|/scale of a level, long double: measured 2.6e-17
TOP_BOUND = 8e-15           # |F+(0) - up[i]|, |F-(t) - diffuse[i+1]| of F0, long double, general: 4.17e-15
TOP_BOUND_CONSERVATIVE = 2.4e-11    # the same in the conservative branch: measured 1.21e-11
GUARD_SLOPE = 0.12          # the header's 0.12*(1e-4 - |1 - k*mu0|) of F0 inside the guard: the
#                             level's own solution, at the moved cosine like the rows: 2.1e-16
ODE_BOUND = 3e-16           # closed-form F+-(tau') against two_stream_ode_cases' solver, of F0,
#                             general: measured 1.46e-16; inside the guard 6.73e-6 (the header's bound)
ODE_BOUND_CONSERVATIVE = 1e-10      # the criterion: the levels tried are conservative exactly, 8.5e-18
SPLIT_BOUND = 1.7e-14       # two halves make the level, of scale, long double: measured 8.26e-15
# Without scattering a level costs the product s*beta, two quotients by a cosine, two exp (their
# argument's rounding times x exp(-x) <= 0.37) and two products: 8 roundings; measured 2.68.
NO_SCATTERING_ROUNDINGS = 8.
THRESHOLD_BOUND = 2.1e-5    # general - conservative at 1 - omega = 1e-6, of scale: measured 1.07e-5
DEPTHS = (1, 2, 9)          # levels per path of the GPU shape tests: 1, 2 and kPathAhead + 1

NO_SCATTERING = 4           # beside two_stream_cases' IDENTITY .. GUARDED: tau_s == 0

# The lines every statement of the definition holds (the header, the docstring of
# compute_solar_radiance, DESIGN section 29 and the head of csrc/solar_radiance.h).
FORMULAS = (
    "Dv = exp(-t/mu) ; a = (3*(gp*mu))/2",
    "source     J(tau') = (w/(2 pi))*[F+(tau')(1 + a) + F-(tau')(1 - a)]",
    "+ ((omega/sc)*Pmix/(4 pi))*(S_i/m)*exp(-tau'/m)",
    "Pmix = (tau_R*PR + w_c*PH)/tau_s ;  PR = (3/4)(1 + cosT^2)",
    "PH = (1 - gc^2)/(1 + gc^2 - 2 gc cosT)^(3/2),  gc = h_c/w_c  (0 where w_c == 0)",
    "ws = w*S_i ; Z+ = (ws*(g3 - a2*m))/X ; Z- = -((ws*(g4 + a1*m))/X)",
    "u1 = up[i+1] - Z+*Dm ; d0 = diffuse[i] - Z-",
    "bm = (m/(m + mu))*(-expm1(-(t/m + t/mu)))",
    "I_top = I_bot*Dv + (w/(2 pi))*C + (((omega/sc)*Pmix)/(4 pi))*((S_i/m)*bm)",
    "Gamma = g2/(g1 + k) ; n = 1 - (Gamma*E)*(Gamma*E)",
    "P = (u1 - (Gamma*E)*d0)/n ; Q = (d0 - (Gamma*E)*u1)/n",
    "C = P*((1 + a) + Gamma*(1 - a))*h + Q*(Gamma*(1 + a) + (1 - a))*((1 - E*Dv)/(1 + k*mu))",
    "+ (Z+*(1 + a) + Z-*(1 - a))*bm",
    "y = ((1 - k*mu)*t)/mu ; phi(z) = -expm1(-z)/z for z > 0, phi(0) = 1",
    "h = E*((t/mu)*phi(y)) for y >= 0 ; h = Dv*((t/mu)*phi(-y)) for y < 0",
    "x = g1*t ; N = (u1 - d0)/(1 + x) ; Ev = -expm1(-t/mu)",
    "C = ((u1 + d0) - x*N + a*N)*Ev + (2*(g1*N))*(mu*W) + (Z+*(1 + a) + Z-*(1 - a))*bm",
    "W = (t/mu)*(Ev - linear_weight(t/mu, Ev))",
    "I_L = A*((direct[L] + diffuse[L])/pi)",
)


def scattering_cosine(mu, mu0, phi):
    """cosT as the host forms it, in float64 and as written, limited to [-1, 1]."""
    mu, mu0, phi = (np.asarray(x, dtype=F64) for x in (mu, mu0, phi))
    value = -mu*mu0 + (np.sqrt((1. - mu)*(1. + mu))*np.sqrt((1. - mu0)*(1. + mu0))) * \
        np.cos(phi*np.pi/180.)
    return np.minimum(np.maximum(value, -1.), 1.)


# ---------------------------------------------------------------------------------------------
# The level.
def view_inputs(table, mu0, beta, sigma):
    """two_stream_cases.layer_inputs with what the view needs beside it, formed in float64 and
    rounded as written: omega/sc, tau_R, tau_s, w_c and gc per element; a level without scattering
    (tau_s == 0 under tau > 0) has the branch NO_SCATTERING."""
    li = dict(ts.layer_inputs(table, mu0, beta, sigma))
    table = np.asarray(table, dtype=F64)
    c, w_c, h_c = table[..., 1], table[..., 3], table[..., 4]
    sigma = np.asarray(sigma, dtype=F64)
    shape = li["branch"].shape
    with np.errstate(all="ignore"):
        tau_r = np.broadcast_to(c*sigma, shape)
        tau_s = tau_r + w_c
        omega = tau_s/li["tau"]
        g = np.where(tau_s == 0., 0., h_c/np.where(tau_s == 0., 1., tau_s))
        sc = 1. - omega*(g*g)
        gc = np.where(w_c == 0., 0., h_c/np.where(w_c == 0., 1., w_c))
    li["branch"] = np.where((li["tau"] != 0.) & (tau_s == 0.), NO_SCATTERING, li["branch"])
    li.update(tau_r=tau_r, tau_s=np.broadcast_to(tau_s, shape), osc=omega/sc,
              w_c=np.broadcast_to(w_c, shape), gc=np.broadcast_to(gc, shape))
    return li


def scalars(kind, li):
    """The level's scalars in `kind` from view_inputs' float64 t, w, gp and branches."""
    one, two, three, four = kind(1.), kind(2.), kind(3.), kind(4.)
    t, w, gp, mu0 = (li[name].astype(kind) for name in ("t", "w", "gp", "mu0"))
    guarded = li["branch"] == ts.GUARDED
    with np.errstate(all="ignore"):
        g2 = (three*(w*(one - gp)))/four
        dif = two*(one - w)
        g1 = g2 + dif
        su = g1 + g2
        g3 = (two - three*(mu0*gp))/four
        g4 = one - g3
        k2 = dif*su
        a1 = g1*g4 + g2*g3
        a2 = g1*g3 + g2*g4
        k = np.sqrt(np.where(k2 > 0., k2, one))
        side = np.where(li["above"], one + kind(ts.RESONANCE), one - kind(ts.RESONANCE))
        m = np.where(guarded, side/k, mu0)
        x = k*m
        big_x = np.where(li["branch"] == ts.CONSERVATIVE_BRANCH, one, (one - x)*(one + x))
        dm = np.exp(-t/m)
        e = np.exp(-(k*t))
    return dict(t=t, w=w, gp=gp, mu0=mu0, g1=g1, g2=g2, g3=g3, g4=g4, a1=a1, a2=a2, k=k, m=m,
                x=big_x, dm=dm, e=e)


def decisions(li, mu):
    """The float64 decisions of the view inside a scattering level: where y >= 0 and where
    linear_weight takes its series."""
    k = scalars(F64, li)["k"]
    mu = np.asarray(mu, dtype=F64)
    with np.errstate(all="ignore"):
        y = ((1. - k*mu)*li["t"])/mu
        z = li["t"]/mu
    return y >= 0., np.abs(z) < rc.LINEAR_SERIES_BELOW


def solution(kind, li, up1, direct0, diffuse0):
    """The two-stream solution inside the level in `kind`: scalars() with Z+ ("zp"), Z- ("zm"),
    u1, d0 and P, Q, Gamma (general) and N (conservative)."""
    one = kind(1.)
    v = scalars(kind, li)
    up1, direct0, diffuse0 = (np.asarray(x, dtype=F64).astype(kind)
                              for x in (up1, direct0, diffuse0))
    with np.errstate(all="ignore"):
        ws = v["w"]*direct0
        zp = (ws*(v["g3"] - v["a2"]*v["m"]))/v["x"]
        zm = -((ws*(v["g4"] + v["a1"]*v["m"]))/v["x"])
        u1 = up1 - zp*v["dm"]
        d0 = diffuse0 - zm
        gamma = v["g2"]/(v["g1"] + v["k"])
        ge = gamma*v["e"]
        n = one - ge*ge
        p = (u1 - ge*d0)/n
        q = (d0 - ge*u1)/n
        big_n = (u1 - d0)/(one + v["g1"]*v["t"])
    v.update(zp=zp, zm=zm, u1=u1, d0=d0, gamma=gamma, p=p, q=q, n=big_n, s=direct0)
    return v


def fields(kind, li, v, depth):
    """(F+, F-) of solution() at tau' = depth (in `kind`, broadcastable), by the closed forms in
    the head of csrc/solar_radiance.h."""
    depth = np.asarray(depth).astype(kind)
    conservative = li["branch"] == ts.CONSERVATIVE_BRANCH
    with np.errstate(all="ignore"):
        beam = np.exp(-depth/v["m"])
        back = np.exp(-(v["k"]*(v["t"] - depth)))
        forth = np.exp(-(v["k"]*depth))
        general = (v["p"]*back + v["gamma"]*v["q"]*forth, v["gamma"]*v["p"]*back + v["q"]*forth)
        linear = (v["u1"] - v["g1"]*v["n"]*(v["t"] - depth), v["d0"] + v["g1"]*v["n"]*depth)
    return tuple(np.where(conservative, linear[i], general[i]) + z*beam
                 for i, z in enumerate((v["zp"], v["zm"])))


def phase(kind, li, cos_theta):
    """Pmix in `kind` from the float64 tau_R, w_c, tau_s and gc."""
    one, two, three, four = kind(1.), kind(2.), kind(3.), kind(4.)
    c = np.asarray(cos_theta, dtype=F64).astype(kind)
    tau_r, w_c, tau_s, gc = (li[name].astype(kind) for name in ("tau_r", "w_c", "tau_s", "gc"))
    with np.errstate(all="ignore"):
        pr = (three*(one + c*c))/four
        den = (one + gc*gc) - (two*gc)*c
        ph = np.where(li["w_c"] == 0., kind(0.), (one - gc*gc)/(den*np.sqrt(den)))
        return (tau_r*pr + w_c*ph)/np.where(li["tau_s"] == 0., one, tau_s)


def source(kind, li, v, mu, cos_theta, depth):
    """J(tau' = depth) of the level in `kind`."""
    one, two, three, four = kind(1.), kind(2.), kind(3.), kind(4.)
    pi = kind(cases.FLUX_PI)
    mu = np.asarray(mu, dtype=F64).astype(kind)
    plus, minus = fields(kind, li, v, depth)
    a = (three*(v["gp"]*mu))/two
    depth = np.asarray(depth).astype(kind)
    return (v["w"]/(two*pi))*(plus*(one + a) + minus*(one - a)) + \
        ((li["osc"].astype(kind)*phase(kind, li, cos_theta))/(four*pi))*(v["s"]/v["m"]) * \
        np.exp(-depth/v["m"])


def level(kind, li, mu, cos_theta, up1, direct0, diffuse0, rad):
    """I at the space-side face of one level from `rad` at its surface-side face, in `kind`:
    li: view_inputs of the level's elements; mu and cos_theta broadcastable to them; up1: the
    float64 up at the level's surface-side interface; direct0, diffuse0: the float64 fluxes at
    its space-side interface."""
    one, two, three, four = kind(1.), kind(2.), kind(3.), kind(4.)
    pi = kind(cases.FLUX_PI)
    branch = li["branch"]
    mu64 = np.asarray(mu, dtype=F64)
    mu = mu64.astype(kind)
    positive, series = decisions(li, mu64)
    v = solution(kind, li, up1, direct0, diffuse0)
    t, m, k, gamma = v["t"], v["m"], v["k"], v["gamma"]
    with np.errstate(all="ignore"):
        z = t/mu
        dv = np.exp(-z)
        a = (three*(v["gp"]*mu))/two
        bm = (m/(m + mu))*(-np.expm1(-(t/m + z)))
        tail = (v["zp"]*(one + a) + v["zm"]*(one - a))*bm
        # Conservative.
        ev = -np.expm1(-z)
        x = v["g1"]*t
        big_w = z*(ev - rc.linear_weight(kind, z, ev, series))
        c_conservative = ((v["u1"] + v["d0"]) - x*v["n"] + a*v["n"])*ev + \
            (two*(v["g1"]*v["n"]))*(mu*big_w) + tail
        # General.
        y = ((one - k*mu)*t)/mu
        h = np.where(positive, v["e"]*(z*rc.phi(kind, np.where(positive, y, 0.))),
                     dv*(z*rc.phi(kind, np.where(positive, 0., -y))))
        c_general = v["p"]*((one + a) + gamma*(one - a))*h + \
            v["q"]*(gamma*(one + a) + (one - a))*((one - v["e"]*dv)/(one + k*mu)) + tail
        c = np.where(branch == ts.CONSERVATIVE_BRANCH, c_conservative, c_general)
        pmix = phase(kind, li, cos_theta)
        scattering = rad*dv + (v["w"]/(two*pi))*c + \
            ((li["osc"].astype(kind)*pmix)/(four*pi))*((v["s"]/m)*bm)
        absorbing = rad*np.exp(-li["tau"].astype(kind)/mu)
    return np.where(branch == ts.IDENTITY, rad,
                    np.where(branch == NO_SCATTERING, absorbing, scattering))


def flux_rows(inputs, from_last):
    """The float64 flux rows lbl_path_two_stream writes for the problem: {"up", "direct",
    "diffuse"} [levels, columns] at the interface below each flat level."""
    fluxes = ts.mirror(F64, inputs, from_last)
    return {q: np.ascontiguousarray(fluxes[q], dtype=F64) for q in ("up", "direct", "diffuse")}


def problem_inputs(inputs, from_last):
    """view_inputs of every element: arrays [L, PATHS, columns] in the Sun's order."""
    order = inputs.sun_order(from_last).T
    return view_inputs(inputs.table[order][:, :, None, :], inputs.mu0[None, :, None],
                       inputs.beta[order], inputs.sigma[None, None, :])


def mirror(kind, inputs, mu, cos_theta, from_last, fluxes=None):
    """{"radiance": I at interface 0 [PATHS, columns] in `kind`, "peak": the largest |I| at the
    path's interfaces} of lbl_path_solar_radiance on a two_stream_cases.Inputs with the view
    cosines mu and the scattering cosines cos_theta [PATHS]; fluxes: flux_rows' (None: formed
    here)."""
    if fluxes is None:
        fluxes = flux_rows(inputs, from_last)
    mu = np.asarray(mu, dtype=F64)[:, None]
    cos_theta = np.asarray(cos_theta, dtype=F64)[:, None]
    order = inputs.sun_order(from_last)                         # [PATHS, L], space -> surface
    li = problem_inputs(inputs, from_last)
    depth = inputs.levels_per_path
    albedo = inputs.albedo[:, None] if inputs.albedo.ndim == 1 else inputs.albedo
    albedo = np.asarray(albedo, dtype=F64).astype(kind)
    pi = kind(cases.FLUX_PI)
    f0 = inputs.f0()
    last = order[:, -1]
    rad = albedo*((fluxes["direct"][last].astype(kind) + fluxes["diffuse"][last].astype(kind))/pi)
    peak = np.abs(rad)
    for i in range(depth - 1, -1, -1):
        here = {name: value[i] for name, value in li.items()}
        direct0 = fluxes["direct"][order[:, i - 1]] if i > 0 else f0
        diffuse0 = fluxes["diffuse"][order[:, i - 1]] if i > 0 else np.zeros_like(f0)
        rad = level(kind, here, mu, cos_theta, fluxes["up"][order[:, i]], direct0, diffuse0, rad)
        peak = np.maximum(peak, np.abs(rad))
    return {"radiance": rad, "peak": peak}


def single_column(kind, table, mu0, beta, sigma, albedo, f0, mu, cos_theta):
    """(I at interface 0, the largest |I| at the interfaces, view_inputs) of independent columns
    [count] through levels [L, count, 5] in the Sun's order, on two_stream_cases' float64 fluxes."""
    li = view_inputs(table, mu0, beta, sigma)
    fluxes = ts.adding(F64, ts.layer(F64, ts.layer_inputs(table, mu0, beta, sigma)), albedo, f0)
    depth = table.shape[0]
    pi = kind(cases.FLUX_PI)
    rad = np.asarray(albedo, dtype=F64).astype(kind) * \
        ((fluxes["direct"][depth].astype(kind) + fluxes["diffuse"][depth].astype(kind))/pi)
    peak = np.abs(rad)
    for i in range(depth - 1, -1, -1):
        here = {name: value[i] for name, value in li.items()}
        rad = level(kind, here, mu, cos_theta, fluxes["up"][i + 1], fluxes["direct"][i],
                    fluxes["diffuse"][i], rad)
        peak = np.maximum(peak, np.abs(rad))
    return rad, peak, li


def scale(inputs, high):
    """[PATHS, columns] in long double from the long-double mirror `high`."""
    return np.maximum(inputs.f0().astype(LD)/LD(cases.FLUX_PI), high["peak"].astype(LD))


def worst_error(inputs, mu, cos_theta, from_last):
    """The worst |float64 mirror - long-double mirror|/scale of the radiance (columns with scale =
    0 must agree exactly), and whether everything is finite."""
    fluxes = flux_rows(inputs, from_last)
    low = mirror(F64, inputs, mu, cos_theta, from_last, fluxes)
    high = mirror(LD, inputs, mu, cos_theta, from_last, fluxes)
    size = scale(inputs, high)
    finite = bool(np.all(np.isfinite(low["radiance"])) and np.all(np.isfinite(high["radiance"])))
    error = np.abs(low["radiance"].astype(LD) - high["radiance"])
    dark = size == 0.
    assert np.all(error[dark] == 0.)
    worst = float(np.max(error[~dark]/size[~dark])) if np.any(~dark) else 0.
    return worst, finite


# ---------------------------------------------------------------------------------------------
# The case tables: two_stream_cases' problems under the views, and the values chosen for the
# branches of the view.
def under_sun(inputs, mu0):
    """`inputs` under other solar zenith cosines."""
    out = ts.Inputs(inputs.name, inputs.beta, inputs.table, mu0, inputs.solar, inputs.sigma,
                    inputs.albedo)
    for name in ("group", "d", "third"):
        if hasattr(inputs, name):
            setattr(out, name, getattr(inputs, name))
    return out


def views():
    """[(mu [PATHS], phi [PATHS])]: every pair of MU and MU0 (MU0[p] is path p's), each phi with
    each of the two."""
    return [(np.roll(MU, r), np.roll(PHI, -r)) for r in range(PATHS)]


def conservative_cloud():
    """omega_c = 1 without gas and without Rayleigh scattering: 4 levels per path on 12 columns,
    tau_c from 1e-6 to 50, g_c up to 0.85."""
    n, columns = 4, 12
    levels = PATHS*n
    tau_c = np.tile([1e-6, 0.3, 5., 50.], PATHS)
    g_c = np.tile([0., 0.85, 0.5, 0.7], PATHS)
    table = np.stack([np.ones(levels), np.zeros(levels), tau_c, tau_c, tau_c*g_c], axis=1)
    return ts.Inputs("conservative cloud", np.zeros((levels, columns)), table, MU0,
                     np.linspace(0.2, 1., columns), np.zeros(columns), (0., 0.3, 1.))


def pole():
    """Clouds at every level, 3 levels per path on 36 columns, for the branches of h.  Columns in
    groups j % 3: 0 beta = 0, where every cloud has the same k and path 0 views along mu = 1/k
    exactly (y = 0), path 1 along (1/k)*(1 + 1e-9) and path 2 along (1/k)*(1 - 1e-9); 1 small
    random beta (y on either side of 0); 2 larger random beta."""
    rng = np.random.default_rng(177)
    n, columns = 3, 36
    levels = PATHS*n
    group = np.arange(columns) % 3
    tau_c = np.repeat([2., 0.5, 8.], n)*np.tile([1., 0.1, 3.], PATHS)
    omega_c, g_c = 0.5, 0.25
    beta = 10.**rng.uniform(-3., 0., size=(levels, columns))
    beta[:, group == 0] = 0.
    beta[:, group == 1] *= 1e-3
    w_c = omega_c*tau_c
    table = np.stack([rng.uniform(0.5, 1.5, size=levels), np.zeros(levels), tau_c, w_c, w_c*g_c],
                     axis=1)
    inputs = ts.Inputs("pole", beta, table, MU0, rng.uniform(0.05, 1., size=columns),
                       np.zeros(columns), ts.ALBEDO)
    k = np.unique(scalars(F64, problem_inputs(inputs, False))["k"][:, :, group == 0])
    assert k.size == 1 and k[0] > 1.
    exact = rc.exact_reciprocal(float(k[0]))
    assert exact is not None
    inputs.group, inputs.k = group, float(k[0])
    inputs.mu = np.array([exact, min(exact*(1. + 1e-9), 1.), exact*(1. - 1e-9)])
    return inputs


def deep():
    """Clouds whose k*t reaches 1000 and 1700 (omega_c = 0.02: k is about 1.97), 2 levels per path
    on 12 columns, beta = 0 in the even columns."""
    rng = np.random.default_rng(178)
    n, columns = 2, 12
    levels = PATHS*n
    tau_c = np.array([508., 3., 865., 508., 1., 865.])
    w_c = 0.02*tau_c
    beta = 10.**rng.uniform(-4., -1., size=(levels, columns))
    beta[:, ::2] = 0.
    table = np.stack([np.ones(levels), np.zeros(levels), tau_c, w_c, np.zeros(levels)], axis=1)
    inputs = ts.Inputs("deep", beta, table, MU0, rng.uniform(0.05, 1., size=columns),
                       np.zeros(columns), ts.ALBEDO)
    inputs.mu = np.array([1., 1., 0.9])
    return inputs


def value_cases():
    """[(inputs, mu, phi)]: two_stream_cases' Rayleigh-only table (the identity level, both sides
    of the conservative threshold) and its cloud under MU0 and every view, its resonance table
    (inside the guard k*mu0 = 1) under its own Sun, and the tables above."""
    out = []
    for inputs in (under_sun(ts.rayleigh_only(), MU0), under_sun(ts.cloud(), MU0),
                   ts.resonance(), conservative_cloud()):
        out += [(inputs, mu, phi) for mu, phi in views()]
    for inputs in (pole(), deep()):
        out.append((inputs, inputs.mu, np.array(PHI)))
    return out


def shape_cases():
    """[(inputs, mu, phi, from_last)]: two_stream_cases' shape problems under MU0, MU and PHI."""
    return [(under_sun(inputs, MU0), np.array(MU), np.array(PHI), from_last)
            for inputs, from_last in ts.shape_cases()]


def all_cases():
    return shape_cases() + [(inputs, mu, phi, from_last) for inputs, mu, phi in value_cases()
                            for from_last in (False, True)]


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class SolarRadianceRecorder(ts.TwoStreamRecorder):
    """tests/two_stream_cases.py's engine with the call of compute_solar_radiance."""
    def path_solar_radiance(self, beta, columns, n_paths, levels_per_path, level_begin,
                            level_table, solar_zenith_cosine, view_cosine, scattering_cosine,
                            solar_row, **keywords):
        self.record("path_solar_radiance", beta=beta, columns=columns, n_paths=n_paths,
                    levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table),
                    solar_zenith_cosine=np.asarray(solar_zenith_cosine),
                    view_cosine=np.asarray(view_cosine),
                    scattering_cosine=np.asarray(scattering_cosine), solar_row=solar_row,
                    **self._described(keywords))
