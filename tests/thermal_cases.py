"""What tests/test_thermal_host.py (CPU), tests/test_gpu_thermal_shapes.py and
tests/test_gpu_thermal_flux.py (GPU) share: the definition of Spectroscopy.compute_thermal_flux in
numpy -- the layer of csrc/twostream_thermal.h and the adding recurrences with thermal sources, for
any float type: float64 "as written", numpy.longdouble as the reference -- a stand-in engine with
the call, and the case tables.  Columns, layouts and bands are tests/sweep_cases.py's.

The layer's inputs (t, w, the level scalars f and gp, and the branch decisions: clear,
conservative, general) are formed in float64, as the host and the kernel form them; a reference in
another float type continues from those.  For a clear level t is tau itself and w is 0.

scale[p, j] = pi*max B(nu_j, T) over the level temperatures of path p and its T_s, in long double:
no flux of the path exceeds it, and every bound is a multiple of it.

E_CPU is the worst |float64 mirror - long-double mirror|/scale over every case table of this file,
as tests/test_thermal_host.py measures it; the GPU tests hold every flux to
(4*E_CPU + FLUX_FLOOR)*scale of the long-double mirror."""
import contextlib

import numpy as np

from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import two_stream_cases as two_stream

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
CONSERVATIVE = 1e-10        # kThermalConservative
UP_AHEAD, DOWN_AHEAD = 8, 1  # kThermalUpAhead, kThermalDownAhead
DIFFUSIVITY = 1.66
QUANTITIES = ("up", "down")
NAMES = tuple(prefix + q for prefix in ("", "top_") for q in QUANTITIES)
# The worst error of the float64 mirror over the case tables, relative to scale (see above):
# tests/test_thermal_host.py measures 6.64e-15.
E_CPU = 7e-15
E_CPU_CAP = 1e-10
FLUX_FLOOR = 1e-13
# Bounds of the mirror's properties (tests/test_thermal_host.py), in units of E_CPU*scale, each
# beside what the float64 mirror was measured to reach.
RANGE_BOUND = 0.5           # fluxes inside [0, scale*(1 + RANGE_BOUND*E_CPU)]: measured 0.384
LID_BOUND = 3.              # up = down = piB under an opaque lid: measured 2.2
SPLIT_BOUND = 0.25          # two halves make the layer: measured 0.144
NET_BOUND = 0.125           # a conservative cloud keeps the net flux: measured 0.0677

CLEAR, CONSERVATIVE_BRANCH, GENERAL = 0, 1, 2

# The lines every statement of the definition holds (the header, the docstring of
# compute_thermal_flux, DESIGN section 23 and the head of csrc/twostream_thermal.h).
FORMULAS = (
    "tau_a = s_l*beta ; tau = tau_a + tau_c",
    "clear level (w_c == 0, the same for the whole wavefront):",
    "x = D*tau ; R = 0 ; T = exp(-x) ; em = -expm1(-x)",
    "cloudy level (w_c > 0; f = g_c*g_c and gp = g_c/(1 + g_c) are level scalars):",
    "omega = w_c/tau ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc",
    "g2 = (D*(w*(1 - gp)))/2 ; dif = D*(1 - w) ; g1 = g2 + dif ; su = g1 + g2 ; k2 = dif*su",
    "conservative, where k2*(1 + t*t) <= 1e-10:",
    "x = g1*t ; R = x/(1 + x) ; T = 1/(1 + x) ; em = (dif*t)/(1 + x)",
    "k = sqrt(k2) ; E = exp(-(k*t)) ; E2 = E*E ; o1 = -expm1(-(2*(k*t)))",
    "den = k*(1 + E2) + g1*o1 ; R = (g2*o1)/den ; T = (2*(k*E))/den",
    "em = (k*((1 - E)*(1 - E)) + dif*o1)/den",
    "S = piB(T_l)*em",
    "up, from the surface: Rs[L] = 1 - eps ; U[L] = eps*piB(T_s) ; for i = L-1 .. 0:",
    "m1 = 1/(1 - R_i*Rs[i+1])",
    "U[i] = S_i + T_i*((U[i+1] + Rs[i+1]*S_i)*m1)",
    "Rs[i] = R_i + T_i*((T_i*Rs[i+1])*m1)",
    "down, from space: Dn = 0, Rd = 0 ; at every interface i = 0 .. L:",
    "m2 = 1/(1 - Rd*Rs[i])",
    "down[i] = (Dn + Rd*U[i])*m2 ; up[i] = (U[i] + Rs[i]*Dn)*m2",
    "then through level i: m3 = 1/(1 - Rd*R_i)",
    "Dn = S_i + T_i*((Dn + Rd*S_i)*m3) ; Rd = R_i + T_i*((T_i*Rd)*m3)",
)


# ---------------------------------------------------------------------------------------------
# The layer.
def layer_inputs(table, d, beta):
    """What the kernel forms in float64 before the branches, each rounded as written: a dict of
    t, w, gp, k2, tau and the branch code per element.  table [..., 5] (s_l, tau_c, w_c, g_c,
    T_l) broadcastable to the elements, d the diffusivity factor, beta float64."""
    table = np.asarray(table, dtype=F64)
    s, tau_c, w_c, g_c = (table[..., i] for i in range(4))
    beta, d = np.asarray(beta, dtype=F64), F64(d)
    with np.errstate(all="ignore"):
        tau_a = s*beta
        tau = tau_a + tau_c
        clear = np.broadcast_to(w_c == 0., tau.shape)
        omega = w_c/np.where(clear, 1., tau)
        f = g_c*g_c
        gp = g_c/(1. + g_c)
        sc = 1. - omega*f
        t = sc*tau
        w = ((1. - f)*omega)/sc
        g2 = (d*(w*(1. - gp)))/2.
        dif = d*(1. - w)
        g1 = g2 + dif
        su = g1 + g2
        k2 = dif*su
        conservative = k2*(1. + t*t) <= CONSERVATIVE
    branch = np.where(clear, CLEAR, np.where(conservative, CONSERVATIVE_BRANCH, GENERAL))
    shape = branch.shape
    return {"t": np.where(clear, tau, t), "w": np.where(clear, 0., w),
            "gp": np.broadcast_to(gp, shape), "k2": np.where(clear, 0., k2),
            "tau": np.broadcast_to(tau, shape), "branch": branch, "d": d}


def layer(kind, inputs):
    """(R, T, em) in `kind` from layer_inputs' float64 t, w, gp and branches, every operation
    rounded as written."""
    one, two = kind(1.), kind(2.)
    t, w, gp = (inputs[name].astype(kind) for name in ("t", "w", "gp"))
    d = kind(inputs["d"])
    branch = inputs["branch"]
    with np.errstate(all="ignore"):
        # Clear.
        x = d*t
        clear_t = np.exp(-x)
        clear_em = -np.expm1(-x)
        # Cloudy.
        g2 = (d*(w*(one - gp)))/two
        dif = d*(one - w)
        g1 = g2 + dif
        su = g1 + g2
        k2 = dif*su
        # Conservative.
        x = g1*t
        c_r = x/(one + x)
        c_t = one/(one + x)
        c_em = (dif*t)/(one + x)
        # General.
        k = np.sqrt(np.where(k2 > 0., k2, one))
        e = np.exp(-(k*t))
        e2 = e*e
        o1 = -np.expm1(-(two*(k*t)))
        den = k*(one + e2) + g1*o1
        r = (g2*o1)/den
        tr = (two*(k*e))/den
        em = (k*((one - e)*(one - e)) + dif*o1)/den

    def pick(clear, conservative, general):
        return np.where(branch == CLEAR, clear,
                        np.where(branch == CONSERVATIVE_BRANCH, conservative, general))
    return pick(kind(0.), c_r, r), pick(clear_t, c_t, tr), pick(clear_em, c_em, em)


def pi_planck(kind, nu, temperature):
    """piB(T) = kFluxPi*planck(nu, c1nu3, c2nu, T) in `kind`."""
    return kind(cases.FLUX_PI)*cases.planck(kind, nu, temperature)


# ---------------------------------------------------------------------------------------------
# Adding.
def adding(kind, layers, source_b, emissivity, surface_b):
    """The adding recurrences over layers = (R, T, em) of L levels in the order space -> surface
    (each [L, ...]), piB(T_l) [L, ...], eps [...] and piB(T_s) [...]: {"up", "down"} at the L + 1
    interfaces [L + 1, ...] (interface 0 faces space), and "u", "rs"."""
    r, t, em = layers
    levels = r.shape[0]
    one = kind(1.)
    eps = np.broadcast_to(np.asarray(emissivity, dtype=F64).astype(kind), r.shape[1:])
    with np.errstate(all="ignore"):
        s = source_b*em
        u = np.zeros((levels + 1,) + r.shape[1:], dtype=kind)
        rs = np.zeros_like(u)
        rs[levels] = one - eps
        u[levels] = eps*surface_b
        for i in range(levels - 1, -1, -1):
            m1 = one/(one - r[i]*rs[i + 1])
            u[i] = s[i] + t[i]*((u[i + 1] + rs[i + 1]*s[i])*m1)
            rs[i] = r[i] + t[i]*((t[i]*rs[i + 1])*m1)
        out = {name: np.zeros_like(u) for name in QUANTITIES}
        dn = np.zeros(r.shape[1:], dtype=kind)
        rd = np.zeros_like(dn)
        for i in range(levels + 1):
            m2 = one/(one - rd*rs[i])
            out["down"][i] = (dn + rd*u[i])*m2
            out["up"][i] = (u[i] + rs[i]*dn)*m2
            if i == levels:
                break
            m3 = one/(one - rd*r[i])
            dn = s[i] + t[i]*((dn + rd*s[i])*m3)
            rd = r[i] + t[i]*((t[i]*rd)*m3)
    out["u"], out["rs"] = u, rs
    return out


def column(kind, table, d, beta, nu, emissivity, surface_t):
    """One or more columns in the order space -> surface: table [L, 5] or [L, n, 5], beta [L, n],
    nu [n] or a scalar, emissivity and surface_t scalars or [n]; adding()'s result, and the layer
    inputs."""
    table = np.asarray(table, dtype=F64)
    beta = np.asarray(beta, dtype=F64)
    if table.ndim == 2:
        table = table[:, None, :]
    inputs = layer_inputs(table, d, beta)
    source_b = pi_planck(kind, nu, table[..., 4])
    surface_b = pi_planck(kind, nu, np.asarray(surface_t, dtype=F64))
    return adding(kind, layer(kind, inputs), source_b, emissivity, surface_b), inputs


# ---------------------------------------------------------------------------------------------
# A problem of PATHS paths in flat storage, as lbl_path_thermal_two_stream takes it.
class Inputs(object):
    """nu [columns], beta [levels, columns], table [levels, 5], the diffusivity factor, surface_t
    [PATHS], emissivity [PATHS] or [PATHS, columns]."""
    def __init__(self, name, nu, beta, table, surface_t, emissivity, diffusivity=DIFFUSIVITY):
        self.name = name
        self.nu = np.ascontiguousarray(nu, dtype=F64)
        self.beta = np.ascontiguousarray(beta, dtype=F64)
        self.table = np.ascontiguousarray(table, dtype=F64)
        self.surface_t = np.asarray(surface_t, dtype=F64)
        self.emissivity = np.asarray(emissivity, dtype=F64)
        self.diffusivity = float(diffusivity)
        self.levels, self.columns = self.beta.shape
        self.levels_per_path = self.levels//PATHS
        assert self.table.shape == (self.levels, 5) and self.levels % PATHS == 0
        assert self.nu.shape == (self.columns,)

    def order(self, from_last):
        """[PATHS, L] flat levels, each path's in the order space -> surface."""
        n = self.levels_per_path
        flat = np.arange(self.levels).reshape(PATHS, n)
        return flat[:, ::-1] if from_last else flat

    def layer_inputs(self, from_last):
        """layer_inputs of every element: arrays [L, PATHS, columns], space -> surface."""
        order = self.order(from_last).T                          # [L, PATHS]
        return layer_inputs(self.table[order][:, :, None, :], self.diffusivity, self.beta[order])

    def scale(self):
        """[PATHS, columns] in long double."""
        n = self.levels_per_path
        temperatures = np.concatenate([self.table[:, 4].reshape(PATHS, n),
                                       self.surface_t[:, None]], axis=1)
        return np.max(pi_planck(LD, self.nu[None, None, :], temperatures[:, :, None]), axis=1)


def mirror(kind, inputs, from_last):
    """{quantity: [levels, columns] at the interface below each flat level, "top_" + quantity:
    [PATHS, columns] at interface 0, "u" and "rs": [levels, columns] at the interface above each
    flat level (the work rows)} in `kind`; "scale" [PATHS, columns] in long double."""
    order = inputs.order(from_last).T
    eps = inputs.emissivity[:, None] if inputs.emissivity.ndim == 1 else inputs.emissivity
    source_b = pi_planck(kind, inputs.nu[None, None, :], inputs.table[order][:, :, None, 4])
    surface_b = pi_planck(kind, inputs.nu[None, :], inputs.surface_t[:, None])
    result = adding(kind, layer(kind, inputs.layer_inputs(from_last)), source_b, eps, surface_b)
    out = {"scale": inputs.scale()}
    for q in QUANTITIES:
        below = np.zeros((inputs.levels, inputs.columns), dtype=kind)
        below[order] = result[q][1:]
        out[q], out["top_" + q] = below, result[q][0]
    for q in ("u", "rs"):
        above = np.zeros((inputs.levels, inputs.columns), dtype=kind)
        above[order] = result[q][:-1]
        out[q] = above
    return out


def per_level(inputs, scale):
    return np.repeat(scale, inputs.levels_per_path, axis=0)


def worst_error(inputs, from_last):
    """The worst |float64 mirror - long-double mirror|/scale of the fluxes at every interface
    (columns with scale = 0 must agree exactly), and whether everything is finite."""
    low, high = mirror(F64, inputs, from_last), mirror(LD, inputs, from_last)
    scale = low["scale"]
    worst, finite = 0., True
    for name in NAMES:
        size = scale if name.startswith("top_") else per_level(inputs, scale)
        finite = finite and bool(np.all(np.isfinite(low[name])))
        error = np.abs(low[name].astype(LD) - high[name])
        dark = size == 0.
        assert np.all(error[dark] == 0.)
        if np.any(~dark):
            worst = max(worst, float(np.max(error[~dark]/size[~dark])))
    return worst, finite


# ---------------------------------------------------------------------------------------------
# The case tables.
# Every loop of path_levels with the eight rows in flight going up (16: two full batches); going
# down one row is in flight: 1, A', A' + 1, 2A' and 2A' + 1 are 1, 2 and 3.
DEPTHS = (1, 2, 3, 8, 9, 16, 17)
SURFACE_T = (270., 288., 305.)
EMISSIVITY = (1., 0.3, 0.)


def shape_inputs(columns, depth, seed, emissivity_rows=False):
    """A problem for the shapes: sweep_cases.Problem's grid (nu from 0 to ~3000 cm-1), beta
    (1e-12 .. 10 m-1 with zeros), thicknesses (one of them 0) and temperatures; cloudy and clear
    levels alternate (which of the two comes first changes from path to path), the clouds with
    omega_c in {1, 0.999999, random} and g_c up to 0.85, every third clear level a grey absorber
    (tau_c > 0 under w_c = 0)."""
    problem = cases.Problem(columns, depth, seed=seed)
    rng = np.random.default_rng(seed + 2000)
    levels = problem.levels
    index = np.arange(levels)
    cloudy = (index % depth + index//depth) % 2 == 0
    tau_c = 10.**rng.uniform(-3., 1.5, size=levels)
    omega_c = rng.choice([1., 0.999999, 0.5], size=levels)
    omega_c = np.where(omega_c == 0.5, rng.uniform(0.05, 1., size=levels), omega_c)
    omega_c = np.where(cloudy, omega_c, 0.)
    tau_c = np.where(cloudy | (index % 3 == 0), tau_c, 0.)
    g_c = rng.choice([0., 0.85, 0.5], size=levels)
    g_c = np.where(g_c == 0.5, rng.uniform(0., 0.85, size=levels), g_c)
    table = np.stack([problem.thickness, tau_c, omega_c*tau_c, g_c, problem.temperature], axis=1)
    emissivity = np.array(EMISSIVITY)
    if emissivity_rows:
        emissivity = rng.uniform(0., 1., size=(PATHS, columns))
        emissivity[0], emissivity[2, ::3] = 1., 0.
    inputs = Inputs("shape %d x %d" % (columns, depth), problem.nu, problem.beta, table, SURFACE_T,
                    emissivity)
    inputs.cloudy = cloudy
    return inputs


CLOUD_PLACES = ("first", "last", "every")


def cloud(place, diffusivity=DIFFUSIVITY):
    """Clouds at the first level of every path, at the last, or at every level, 9 levels per path
    on 68 columns, nu from 1 to 3000 cm-1, T_l from 180 to 320 K.  The clouds take omega_c from
    (1, 0.5, 0.999999) and g_c from (0, 0.85) in turn, tau_c from 1e-3 to 30 and, in path 1, 3000.
    Columns in groups j % 4: 0 beta = 0 (under omega_c = 1: k2 = 0 exactly; in a clear level
    without tau_c: the identity layer, x = 0); 1 beta = delta*tau_c/s with delta*(1 + tau_c^2) from
    1e-13 to 1e-8, so that under omega_c = 1 k2*(1 + t*t) lies on both sides of 1e-10; 2 s*beta =
    3000 in each path's first and last level; 3 random beta."""
    rng = np.random.default_rng(31 + CLOUD_PLACES.index(place))
    n, columns = 9, 68
    levels = PATHS*n
    group = np.arange(columns) % 4
    index = np.arange(levels)
    cloudy = {"first": index % n == 0, "last": index % n == n - 1,
              "every": np.ones(levels, dtype=bool)}[place]
    thickness = rng.uniform(0.5, 1.5, size=levels)
    temperature = rng.permutation(np.linspace(180., 320., levels))
    tau_c = np.where(cloudy, 10.**rng.uniform(-3., np.log10(30.), size=levels), 0.)
    tau_c[(index//n == 1) & cloudy & (index % 2 == 0)] = 3000.
    omega_c = np.where(cloudy, np.array([1., 0.5, 0.999999])[index % 3], 0.)
    if place != "every":
        # One cloud per path: path p takes omega_c = (1, 0.5, 0.999999)[p].
        omega_c = np.where(cloudy, np.array([1., 0.5, 0.999999])[index//n], 0.)
    g_c = np.array([0., 0.85])[(index + index//n) % 2]
    beta = 10.**rng.uniform(-6., 0.5, size=(levels, columns))
    beta[:, group == 0] = 0.
    near = np.where(cloudy, tau_c, 1.)
    delta = 10.**np.linspace(-13., -8., int(np.sum(group == 1)))[None, :]/(1. + near*near)[:, None]
    beta[:, group == 1] = delta*near[:, None]/thickness[:, None]
    for p in range(PATHS):
        for level in (n*p, n*p + n - 1):
            beta[level, group == 2] = 3000./thickness[level]
    table = np.stack([thickness, tau_c, omega_c*tau_c, g_c, temperature], axis=1)
    inputs = Inputs("cloud at %s" % place, np.linspace(1., 3000., columns), beta, table,
                    (250., 288., 320.), EMISSIVITY, diffusivity)
    inputs.group, inputs.omega_c, inputs.cloudy = group, omega_c, cloudy
    return inputs


def value_cases():
    return [cloud(place) for place in CLOUD_PLACES] + [cloud("every", 2.), cloud("every", 1.)]


def shape_cases():
    """Every problem the shape tests run: [(inputs, from_last)]."""
    out = []
    for columns in cases.LAYOUT_COLUMNS:
        out.append((shape_inputs(columns, 9, columns), True))
    for depth in DEPTHS:
        for from_last in (False, True):
            out.append((shape_inputs(513, depth, 40 + depth, emissivity_rows=True), from_last))
    for _, columns, _ in cases.BAND_SETS:
        out.append((shape_inputs(columns, 3, 70), True))
    return out


def all_cases():
    return shape_cases() + [(inputs, from_last) for inputs in value_cases()
                            for from_last in (False, True)]


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class ThermalRecorder(two_stream.TwoStreamRecorder):
    """tests/two_stream_cases.py's engine with the call of compute_thermal_flux."""
    def path_thermal_two_stream(self, beta, columns, grid, n_paths, levels_per_path, level_begin,
                                level_table, surface_temperature, work, **keywords):
        self.record("path_thermal_two_stream", beta=beta, columns=columns, grid=grid,
                    n_paths=n_paths, levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table),
                    surface_temperature=np.asarray(surface_temperature), work=work,
                    **self._described(keywords))


@contextlib.contextmanager
def recorded(directory):
    """surface_cases.recorded with a ThermalRecorder."""
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = ThermalRecorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before
