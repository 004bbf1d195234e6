"""What tests/test_thermal_radiance_host.py (CPU), tests/test_gpu_thermal_radiance_shapes.py and
tests/test_gpu_thermal_radiance.py (GPU) share: the definition of
Spectroscopy.compute_thermal_radiance in numpy -- the level of csrc/thermal_radiance.h, for any
float type: float64 "as written", numpy.longdouble as the reference -- and the case tables.  The
layer inputs, the two-stream fluxes and the problems are tests/thermal_cases.py's.

Like thermal_cases' mirror this one continues from the float64 layer inputs (t, w, gp) and the
float64 branch decisions: clear, conservative or general, the side of y = 0 and the branch of
linear_weight.  The flux rows are inputs of the kernel: both float types read the same float64
rows, the float64 mirror of thermal_cases.

scale[p, j] = max B(nu_j, T) over the level temperatures of path p and its T_s, in long double: no
radiance of the path exceeds it, and every bound is a multiple of it.

E_CPU is the worst |float64 mirror - long-double mirror|/scale over every case table of this file,
as tests/test_thermal_radiance_host.py measures it; the GPU tests hold every radiance to
(4*E_CPU + FLOOR)*scale of the long-double mirror."""
import numpy as np

from tests import sweep_cases as cases
from tests import thermal_cases as tc

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
VIEW_AHEAD = 1              # kThermalViewAhead
LINEAR_SERIES_BELOW = 1./16.    # kLinearSeriesBelow of csrc/radiance.h
MU = (1., 0.6, 0.05)
# The worst error of the float64 mirror over the case tables, relative to scale (see above):
# tests/test_thermal_radiance_host.py measures 1.9e-11, in the general branch just above the
# conservative threshold, where n = 1 - (Gamma*E)*(Gamma*E) is a difference of nearly equal
# numbers (n is about 1e-5 there) that P and Q are divided by.
E_CPU = 2e-11
E_CPU_CAP = 1e-10
FLOOR = 1e-13
# Bounds of the mirror's properties (tests/test_thermal_radiance_host.py), each beside what was
# measured there.
QUADRATURE_BOUND = 9e-17    # |C - quadrature|/(|u1| + |d0|), long double: measured 4.6e-17
TOP_BOUND = 6.5e-15         # |f+(0) - (up[i] - piB)|/(pi*scale), long double, general: 3.29e-15
TOP_BOUND_CONSERVATIVE = 2.8e-11    # the same in the conservative branch: measured 1.4e-11
SPLIT_BOUND = 1.2e-4        # two halves make the level, in E_CPU*scale: measured 6.05e-5
RANGE_BOUND = 0.            # radiances inside [0, scale*(1 + RANGE_BOUND*E_CPU)]: measured 0
THRESHOLD_BOUND = 1.9e-5    # general - conservative at 1 - omega = 1e-6, of scale: 9.45e-6

# The lines every statement of the definition holds (the header, the docstring of
# compute_thermal_radiance, DESIGN section 27 and the head of csrc/thermal_radiance.h).
FORMULAS = (
    "gp = g_c/(1 + g_c) ; a = (3*(gp*mu))/2",
    "u1 = up[i+1] - piB ; d0 = down[i] - piB ; Dm = exp(-t/mu) ; Em = -expm1(-t/mu)",
    "I_top = I_bot*Dm + B*Em + (w/(2 pi))*C",
    "x = tau/mu and C = 0:",
    "I_top = I_bot*exp(-x) + B*(-expm1(-x))",
    "Gamma = g2/(g1 + k) ; n = 1 - (Gamma*E)*(Gamma*E)",
    "P = (u1 - (Gamma*E)*d0)/n ; Q = (d0 - (Gamma*E)*u1)/n",
    "C = P*((1 + a) + Gamma*(1 - a))*h + Q*(Gamma*(1 + a) + (1 - a))*((1 - E*Dm)/(1 + k*mu))",
    "y = ((1 - k*mu)*t)/mu ; phi(z) = -expm1(-z)/z for z > 0, phi(0) = 1",
    "h = E*((t/mu)*phi(y)) for y >= 0 ; h = Dm*((t/mu)*phi(-y)) for y < 0",
    "x = g1*t ; N = (u1 - d0)/(1 + x)",
    "C = ((u1 + d0) - x*N + a*N)*Em + (2*(g1*N))*(mu*W)",
    "W = (t/mu)*(Em - linear_weight(t/mu, Em))",
    "I_L = eps*B(T_s) + (1 - eps)*(down[L]/pi)",
)


# ---------------------------------------------------------------------------------------------
# The level.
def linear_weight(kind, x, a, series):
    """csrc/radiance.h's linear_weight in `kind`: w = 1 - a/x, by its series where `series`."""
    one = kind(1.)
    x, a = np.asarray(x, dtype=kind), np.asarray(a, dtype=kind)
    c = [one/kind(f) for f in (2., 6., 24., 120., 720., 5040., 40320., 362880.)]
    with np.errstate(all="ignore"):
        horner = x*(c[0] - x*(c[1] - x*(c[2] - x*(c[3] - x*(c[4] - x*(c[5] - x*(c[6] - x*c[7])))))))
        direct = one - a/np.where(x == 0., one, x)
    return np.where(series, horner, direct)


def phi(kind, z):
    """phi(z) = -expm1(-z)/z for z > 0, 1 at z = 0."""
    z = np.asarray(z, dtype=kind)
    with np.errstate(all="ignore"):
        value = -np.expm1(-z)/np.where(z > 0., z, kind(1.))
    return np.where(z > 0., value, kind(1.))


def general_c(kind, k, gamma, t, mu, a, u1, d0, positive=None):
    """(C, P, Q, E) of the general branch in `kind`.  positive: where y >= 0 (None: decided in
    `kind`)."""
    one = kind(1.)
    k, gamma, t, mu, a, u1, d0 = (np.asarray(x, dtype=kind) for x in (k, gamma, t, mu, a, u1, d0))
    with np.errstate(all="ignore"):
        z = t/mu
        dm = np.exp(-z)
        e = np.exp(-(k*t))
        ge = gamma*e
        n = one - ge*ge
        p = (u1 - ge*d0)/n
        q = (d0 - ge*u1)/n
        y = ((one - k*mu)*t)/mu
        if positive is None:
            positive = y >= 0.
        h = np.where(positive, e*(z*phi(kind, np.where(positive, y, 0.))),
                     dm*(z*phi(kind, np.where(positive, 0., -y))))
        c = p*((one + a) + gamma*(one - a))*h + \
            q*(gamma*(one + a) + (one - a))*((one - e*dm)/(one + k*mu))
    return c, p, q, e


def conservative_c(kind, g1, t, mu, a, u1, d0, series=None):
    """(C, N) of the conservative branch in `kind`.  series: where linear_weight takes its series
    (None: decided in `kind`)."""
    one, two = kind(1.), kind(2.)
    g1, t, mu, a, u1, d0 = (np.asarray(x, dtype=kind) for x in (g1, t, mu, a, u1, d0))
    with np.errstate(all="ignore"):
        z = t/mu
        dm = np.exp(-z)
        em = -np.expm1(-z)
        x = g1*t
        n = (u1 - d0)/(one + x)
        if series is None:
            series = np.abs(z) < LINEAR_SERIES_BELOW
        big_w = z*(em - linear_weight(kind, z, em, series))
        c = ((u1 + d0) - x*n + a*n)*em + (two*(g1*n))*(mu*big_w)
    del dm
    return c, n


def decisions(inputs, mu):
    """The float64 decisions inside a cloudy level, from layer_inputs' t, w, gp and mu (broadcast
    to the elements): where y >= 0 and where linear_weight takes its series."""
    _, _, k, _ = scalars(F64, inputs)
    mu = np.asarray(mu, dtype=F64)
    with np.errstate(all="ignore"):
        y = ((1. - k*mu)*inputs["t"])/mu
        z = inputs["t"]/mu
    return y >= 0., np.abs(z) < LINEAR_SERIES_BELOW, y


def scalars(kind, inputs):
    """(g1, g2, k, w) of a cloudy level in `kind` from layer_inputs' float64 t, w, gp."""
    one, two = kind(1.), kind(2.)
    w, gp = inputs["w"].astype(kind), inputs["gp"].astype(kind)
    d = kind(inputs["d"])
    with np.errstate(all="ignore"):
        g2 = (d*(w*(one - gp)))/two
        dif = d*(one - w)
        g1 = g2 + dif
        su = g1 + g2
        k2 = dif*su
        k = np.sqrt(np.where(k2 > 0., k2, one))
    return g1, g2, k, w


def level(kind, inputs, mu, b, up1, down0, rad):
    """I at the space-side face of one level from `rad` at its surface-side face, in `kind`:
    inputs: layer_inputs of the level's elements; mu broadcastable to them; b: B(T_l) in `kind`;
    up1, down0: the float64 fluxes at the level's surface-side and space-side interfaces."""
    one, two, three = kind(1.), kind(2.), kind(3.)
    pi = kind(cases.FLUX_PI)
    branch = inputs["branch"]
    t = inputs["t"].astype(kind)
    mu64 = np.asarray(mu, dtype=F64)
    mu = mu64.astype(kind)
    positive, series, _ = decisions(inputs, mu64)
    g1, g2, k, w = scalars(kind, inputs)
    with np.errstate(all="ignore"):
        # Clear: t is tau itself.
        x = t/mu
        clear = rad*np.exp(-x) + b*(-np.expm1(-x))
        # Cloudy.
        a = (three*(inputs["gp"].astype(kind)*mu))/two
        pib = pi*b
        u1 = np.asarray(up1, dtype=F64).astype(kind) - pib
        d0 = np.asarray(down0, dtype=F64).astype(kind) - pib
        dm = np.exp(-x)
        em = -np.expm1(-x)
        gamma = g2/(g1 + k)
        c_general, _, _, _ = general_c(kind, k, gamma, t, mu, a, u1, d0, positive)
        c_conservative, _ = conservative_c(kind, g1, t, mu, a, u1, d0, series)
        c = np.where(branch == tc.CONSERVATIVE_BRANCH, c_conservative, c_general)
        cloudy = rad*dm + b*em + (w/(two*pi))*c
    return np.where(branch == tc.CLEAR, clear, cloudy)


def flux_rows(inputs, from_last):
    """The float64 flux rows lbl_path_thermal_two_stream writes for the problem: {"up", "down"}
    [levels, columns] at the interface below each flat level."""
    fluxes = tc.mirror(F64, inputs, from_last)
    return {q: np.ascontiguousarray(fluxes[q], dtype=F64) for q in tc.QUANTITIES}


def scale(inputs):
    """[PATHS, columns] in long double: max B over the path's level temperatures and T_s."""
    n = inputs.levels_per_path
    temperatures = np.concatenate([inputs.table[:, 4].reshape(PATHS, n),
                                   inputs.surface_t[:, None]], axis=1)
    return np.max(cases.planck(LD, inputs.nu[None, None, :], temperatures[:, :, None]), axis=1)


def mirror(kind, inputs, mu, from_last, fluxes=None):
    """{"radiance", "brightness_temperature": [PATHS, columns] in `kind`, "scale" in long double} of
    lbl_path_thermal_radiance on a thermal_cases.Inputs with the view cosines mu [PATHS];
    fluxes: flux_rows' (None: formed here)."""
    if fluxes is None:
        fluxes = flux_rows(inputs, from_last)
    mu = np.asarray(mu, dtype=F64)
    order = inputs.order(from_last)                             # [PATHS, L], space -> surface
    li = inputs.layer_inputs(from_last)                         # [L, PATHS, columns]
    depth = inputs.levels_per_path
    eps = inputs.emissivity[:, None] if inputs.emissivity.ndim == 1 else inputs.emissivity
    eps = np.asarray(eps, dtype=F64).astype(kind)
    one, pi = kind(1.), kind(cases.FLUX_PI)
    nu = inputs.nu[None, :]
    with np.errstate(all="ignore"):
        surface_down = fluxes["down"][order[:, -1]].astype(kind)
        rad = eps*cases.planck(kind, nu, inputs.surface_t[:, None]) + \
            (one - eps)*(surface_down/pi)
    for i in range(depth - 1, -1, -1):
        here = {name: (value[i] if isinstance(value, np.ndarray) and value.ndim == 3 else value)
                for name, value in li.items()}
        b = cases.planck(kind, nu, inputs.table[order[:, i], 4][:, None])
        down0 = fluxes["down"][order[:, i - 1]] if i > 0 else np.zeros_like(fluxes["down"][:PATHS])
        rad = level(kind, here, mu[:, None], b, fluxes["up"][order[:, i]], down0, rad)
    return {"radiance": rad, "brightness_temperature": cases.brightness(kind, nu, rad),
            "scale": scale(inputs)}


def worst_error(inputs, mu, from_last):
    """The worst |float64 mirror - long-double mirror|/scale of the radiance (columns with scale =
    0 must agree exactly), and whether everything is finite."""
    fluxes = flux_rows(inputs, from_last)
    low, high = mirror(F64, inputs, mu, from_last, fluxes), mirror(LD, inputs, mu, from_last, fluxes)
    size = low["scale"]
    finite = bool(np.all(np.isfinite(low["radiance"])) and np.all(np.isfinite(high["radiance"])))
    error = np.abs(low["radiance"].astype(LD) - high["radiance"])
    dark = size == 0.
    assert np.all(error[dark] == 0.)
    worst = float(np.max(error[~dark]/size[~dark])) if np.any(~dark) else 0.
    return worst, finite


# ---------------------------------------------------------------------------------------------
# The case tables: thermal_cases' problems under the three view cosines, and the values chosen for
# the branches of h.
def exact_reciprocal(k):
    """mu with k*mu == 1 exactly in float64 (k > 1), or None."""
    base = 1./k
    for candidate in (base, np.nextafter(base, 0.), np.nextafter(base, 1.)):
        if k*candidate == 1. and 0. < candidate <= 1.:
            return float(candidate)
    return None


def pole(diffusivity=tc.DIFFUSIVITY):
    """Clouds at every level, 3 levels per path on 36 columns, for the branches of h.  Columns in
    groups j % 3: 0 beta = 0, where every cloud of a path has the same k and path 0 views along mu
    = 1/k exactly (y = 0), path 1 along (1/k)*(1 + 1e-9) and path 2 along (1/k)*(1 - 1e-9); 1 small
    random beta (y on either side of 0); 2 larger random beta."""
    rng = np.random.default_rng(77)
    n, columns = 3, 36
    levels = PATHS*n
    group = np.arange(columns) % 3
    thickness = rng.uniform(0.5, 1.5, size=levels)
    temperature = np.linspace(200., 300., levels)
    tau_c = np.repeat([2., 0.5, 8.], n)*np.tile([1., 0.1, 3.], PATHS)
    omega_c, g_c = 0.5, 0.25
    beta = 10.**rng.uniform(-3., 0., size=(levels, columns))
    beta[:, group == 0] = 0.
    beta[:, group == 1] *= 1e-3
    table = np.stack([thickness, tau_c, omega_c*tau_c, np.full(levels, g_c), temperature], axis=1)
    inputs = tc.Inputs("pole", np.linspace(50., 2500., columns), beta, table, (250., 288., 320.),
                       tc.EMISSIVITY, diffusivity)
    li = inputs.layer_inputs(False)
    _, _, k, _ = scalars(F64, li)
    k = np.unique(k[:, :, group == 0])
    assert k.size == 1 and k[0] > 1.
    exact = exact_reciprocal(float(k[0]))
    assert exact is not None
    inputs.group, inputs.k = group, float(k[0])
    inputs.mu = np.array([exact, min(exact*(1. + 1e-9), 1.), exact*(1. - 1e-9)])
    return inputs


def deep(diffusivity=2.):
    """Clouds whose k*t reaches 1000 and 1700 under mu = 1 (D = 2, omega_c = 0.02: k is about
    1.98, so y = -(k - 1)*t is about -490 and -840: E underflows, and at -840 expm1(-y) overflows),
    2 levels per path on 12 columns, beta = 0 in the even columns."""
    rng = np.random.default_rng(78)
    n, columns = 2, 12
    levels = PATHS*n
    thickness = np.ones(levels)
    temperature = np.linspace(220., 300., levels)
    tau_c = np.array([505., 3., 860., 505., 1., 860.])
    omega_c = 0.02
    beta = 10.**rng.uniform(-4., -1., size=(levels, columns))
    beta[:, ::2] = 0.
    table = np.stack([thickness, tau_c, omega_c*tau_c, np.zeros(levels), temperature], axis=1)
    inputs = tc.Inputs("deep", np.linspace(100., 2000., columns), beta, table, (250., 288., 320.),
                       tc.EMISSIVITY, diffusivity)
    inputs.mu = np.array([1., 1., 0.9])
    return inputs


def value_cases():
    """[(inputs, mu)]: thermal_cases' clouds at the first level, at the last and at every level
    (both sides of the conservative threshold, tau = 3000, the identity layer) under MU, and the
    two tables above."""
    out = [(inputs, np.array(MU)) for inputs in tc.value_cases()]
    for inputs in (pole(), deep()):
        out.append((inputs, inputs.mu))
    return out


def shape_cases():
    """[(inputs, mu, from_last)]: thermal_cases' shape problems under MU."""
    return [(inputs, np.array(MU), from_last) for inputs, from_last in tc.shape_cases()]


def all_cases():
    return shape_cases() + [(inputs, mu, from_last) for inputs, mu in value_cases()
                            for from_last in (False, True)]


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class RadianceRecorder(tc.ThermalRecorder):
    """tests/thermal_cases.py's engine with the call of compute_thermal_radiance."""
    def path_thermal_radiance(self, beta, columns, grid, n_paths, levels_per_path, level_begin,
                              level_table, view_cosine, surface_temperature, **keywords):
        self.record("path_thermal_radiance", beta=beta, columns=columns, grid=grid,
                    n_paths=n_paths, levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table), view_cosine=np.asarray(view_cosine),
                    surface_temperature=np.asarray(surface_temperature),
                    **self._described(keywords))
