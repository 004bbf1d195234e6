"""What tests/test_thermal_source_host.py (CPU), tests/test_gpu_thermal_source_shapes.py and
tests/test_gpu_thermal_flux_linear.py (GPU) share: the definition of
Spectroscopy.compute_thermal_flux_linear in numpy -- tests/thermal_cases.py's layer with the weight
q of csrc/twostream_thermal_source.h and the adding recurrences with the two sources S_up and S_dn,
for any float type: float64 "as written", numpy.longdouble as the reference -- a stand-in engine
with the call, and the case tables.

As in tests/thermal_cases.py both mirrors continue from the float64 layer inputs and the float64
branch decisions (clear, conservative, general, and y = k*t against Y0).  The long-double q takes
its p from a longer series below Y0 and from the direct form above, and the clear weight from
tests/linear_source_cases.py's 24-term reference.

scale[p, j] = pi*max B(nu_j, T) over the interface temperatures of path p and its T_s, in long
double: every bound is a multiple of it.

E_CPU is the worst |float64 mirror - long-double mirror|/scale over every case table of this file,
as tests/test_thermal_source_host.py measures it; the GPU tests hold every flux to
(4*E_CPU + FLUX_FLOOR)*scale of the long-double mirror."""
import contextlib
import math

import numpy as np

from tests import linear_source_cases as ls
from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import thermal_cases as tc

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
Y0 = 0.5                    # kThermalSourceSeriesBelow
SERIES_TERMS = 8            # of p in float64, as the kernel has them
REFERENCE_TERMS = 14        # of p in long double
UP_AHEAD, DOWN_AHEAD = 1, 1  # kThermalSourceUpAhead, kThermalSourceDownAhead
QUANTITIES, NAMES = tc.QUANTITIES, tc.NAMES
# The worst relative error of the float64 q against the long-double q over y from 1e-8 to 50 and
# su*t from 1e-6 to 1e3 (tests/test_thermal_source_host.py measures 4.69e-15, at y just above Y0,
# where the direct p has lost a factor of about 25), beside the 1.5e-14 of the clear weight
# (DESIGN section 18), which is the yardstick: the bound is that figure.
Q_ERROR = 4.7e-15
Q_BOUND = 1.5e-14
# The worst error of the float64 mirror over the case tables, relative to scale:
# tests/test_thermal_source_host.py measures 4.73e-15.
E_CPU = 5e-15
E_CPU_CAP = 1e-10
FLUX_FLOOR = 1e-13
# Bounds of the mirror's properties (tests/test_thermal_source_host.py), in units of E_CPU*scale,
# each beside what the float64 mirror was measured to reach.
# Two halves with the midpoint source make the layer: twice thermal_cases.SPLIT_BOUND, for the two
# sources a level has here where it has one there.  Measured 0.118.
SPLIT_BOUND = 0.5
# Bb - dB/x leaves a clear layer of tau = 1e3 downward.  The float64 Planck value is off by up to
# (2*c + 6)*2^-53 relative, c = C2*nu/T <= 1.4388*3000/180 = 24 (two roundings of the argument,
# which expm1 amplifies by c, then expm1, the three products of C1*nu^3, the quotient and pi), and
# the source adds four roundings: 58*2^-53 = 6.4e-15, under 1.5*E_CPU.  Measured 0.638.
THICK_BOUND = 1.5
# The relative gap between the conservative q and the long-double general q where
# k2*(1 + t*t) is 1e-10 (the conservative q is the first-order limit in k): measured 2.89e-11; the
# bound is the criterion itself, k2*(1 + t*t), whose order the neglected terms (y*y/6 and the
# like) have.
JOIN_GAP = 2.9e-11
JOIN_BOUND = 1e-10
# Without scatterers, against lbl_path_flux_source's recurrence with the one angle mu = 1/D: the
# 16*2^-53*(L + 1)*scale of tests/test_thermal_host.py (x = D*(s*beta) against (s/mu)*beta, and
# where pi enters) and, per level and sweep, four more roundings of 2^-53*scale where the weight
# enters: dB*q and Bt*em + dB*q against B_in*(a - w) + B_out*w (the same q = a - w and the same
# Planck values, otherwise associated: a product, a sum, a difference and the pi of each term),
# two sweeps: 24*2^-53*(L + 1)*scale.  Measured: 0.048 of it at worst.
PLAIN_ROUNDINGS = 24.

# The lines every statement of the definition holds beside thermal_cases.FORMULAS' layer (the
# header, the docstring of compute_thermal_flux_linear, DESIGN section 25 and the head of
# csrc/twostream_thermal_source.h).
FORMULAS = (
    "S_up = Bt*em + dB*q",
    "S_dn = Bb*em - dB*q",
    "q = a - linear_weight(x, a)",
    "y = k*t ; z = y*y",
    "p = o1 - 2*(y*E)",
    "p = E*(((y*z)/3)*(1 + z*(1/20 + z*(1/840 + z*(1/60480 + z*(1/6652800 + z*(1/1037836800 + "
    "z*(1/217945728000 + z*(1/59281238016000)))))))))",
    "q = ((k*(o1*o1))/(su*((1 + E)*(1 + E))) + p)/(den*t)",
    "q = ((dif*t)*(1 + (su*t)/3))/(2*(1 + x))",
    "U[i] = S_up_i + T_i*((U[i+1] + Rs[i+1]*S_dn_i)*m1)",
    "Dn = S_dn_i + T_i*((Dn + Rd*S_up_i)*m3)",
)


# ---------------------------------------------------------------------------------------------
# The weight.
def p_series(kind, y, e, terms):
    """E*(((y*z)/3)*(1 + z*(1/20 + ...))) in `kind` with `terms` terms: coefficient n is
    6/(2n + 3)! (n = 0: 1)."""
    z = y*y
    series = np.zeros(np.shape(y), dtype=kind)
    for n in range(terms - 1, 0, -1):
        series = z*(kind(1.)/kind(math.factorial(2*n + 3)//6) + series)
    series = kind(1.) + series
    return e*(((y*z)/kind(3.))*series)


def general_q(kind, k, t, su, g1, below, terms):
    """The general q in `kind` from k, t, su and g1 in `kind`; `below`: where p comes from its
    series."""
    one, two = kind(1.), kind(2.)
    with np.errstate(all="ignore"):
        y = k*t
        e = np.exp(-y)
        e2 = e*e
        o1 = -np.expm1(-(two*y))
        den = k*(one + e2) + g1*o1
        p = np.where(below, p_series(kind, y, e, terms), o1 - two*(y*e))
        return ((k*(o1*o1))/(su*((one + e)*(one + e))) + p)/(den*t)


def weight(kind, inputs):
    """q in `kind` from thermal_cases.layer_inputs' float64 t, w, gp and branches, every operation
    rounded as written."""
    one, two = kind(1.), kind(2.)
    t, w, gp = (inputs[name].astype(kind) for name in ("t", "w", "gp"))
    d = kind(inputs["d"])
    branch = inputs["branch"]
    with np.errstate(all="ignore"):
        # The float64 decision between the two forms of p.
        k64 = np.sqrt(np.where(inputs["k2"] > 0., inputs["k2"], 1.))
        below = k64*inputs["t"] < Y0
        # Clear.
        x = d*t
        a = -np.expm1(-x)
        clear = a - (ls.device_weight(x) if kind is F64 else ls.weight(kind, x))
        # Cloudy.
        g2 = (d*(w*(one - gp)))/two
        dif = d*(one - w)
        g1 = g2 + dif
        su = g1 + g2
        k2 = dif*su
        x = g1*t
        conservative = ((dif*t)*(one + (su*t)/kind(3.)))/(two*(one + x))
        k = np.sqrt(np.where(k2 > 0., k2, one))
        general = general_q(kind, k, t, su, g1, below,
                            SERIES_TERMS if kind is F64 else REFERENCE_TERMS)
    return np.where(branch == tc.CLEAR, clear,
                    np.where(branch == tc.CONSERVATIVE_BRANCH, conservative, general))


# ---------------------------------------------------------------------------------------------
# Adding.
def adding(kind, layers, q, bt, bb, emissivity, surface_b):
    """thermal_cases.adding with the two sources: layers = (R, T, em) and q of L levels in the
    order space -> surface (each [L, ...]), bt and bb = piB at each level's space-side and
    surface-side interface [L, ...], eps [...] and piB(T_s) [...]."""
    r, t, em = layers
    levels = r.shape[0]
    one = kind(1.)
    eps = np.broadcast_to(np.asarray(emissivity, dtype=F64).astype(kind), r.shape[1:])
    with np.errstate(all="ignore"):
        db = bb - bt
        s_up = bt*em + db*q
        s_dn = bb*em - db*q
        u = np.zeros((levels + 1,) + r.shape[1:], dtype=kind)
        rs = np.zeros_like(u)
        rs[levels] = one - eps
        u[levels] = eps*surface_b
        for i in range(levels - 1, -1, -1):
            m1 = one/(one - r[i]*rs[i + 1])
            u[i] = s_up[i] + t[i]*((u[i + 1] + rs[i + 1]*s_dn[i])*m1)
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
            dn = s_dn[i] + t[i]*((dn + rd*s_up[i])*m3)
            rd = r[i] + t[i]*((t[i]*rd)*m3)
    out["u"], out["rs"] = u, rs
    return out


def column(kind, table, d, beta, nu, interfaces, emissivity, surface_t):
    """One or more columns in the order space -> surface: table [L, 5] or [L, n, 5], beta [L, n],
    nu [n] or a scalar, interfaces [L + 1] or [L + 1, n] (0 facing space), emissivity and
    surface_t scalars or [n]; adding()'s result, and the layer inputs."""
    table = np.asarray(table, dtype=F64)
    beta = np.asarray(beta, dtype=F64)
    if table.ndim == 2:
        table = table[:, None, :]
    interfaces = np.asarray(interfaces, dtype=F64)
    if interfaces.ndim == 1:
        interfaces = interfaces[:, None]
    inputs = tc.layer_inputs(table, d, beta)
    bt = tc.pi_planck(kind, nu, interfaces[:-1])
    bb = tc.pi_planck(kind, nu, interfaces[1:])
    surface_b = tc.pi_planck(kind, nu, np.asarray(surface_t, dtype=F64))
    return adding(kind, tc.layer(kind, inputs), weight(kind, inputs), bt, bb, emissivity,
                  surface_b), inputs


# ---------------------------------------------------------------------------------------------
# A problem of PATHS paths in flat storage, as lbl_path_thermal_two_stream_source takes it.
class Inputs(tc.Inputs):
    """thermal_cases.Inputs with interfaces [PATHS, L + 1]: the temperature of interface l of a
    path, between its levels l - 1 and l in storage order."""
    def __init__(self, name, nu, beta, table, interfaces, surface_t, emissivity,
                 diffusivity=tc.DIFFUSIVITY):
        tc.Inputs.__init__(self, name, nu, beta, table, surface_t, emissivity, diffusivity)
        self.interfaces = np.ascontiguousarray(interfaces, dtype=F64)
        assert self.interfaces.shape == (PATHS, self.levels_per_path + 1)
        self.edges = ls.edge_table(self.interfaces)

    def scale(self):
        """[PATHS, columns] in long double."""
        temperatures = np.concatenate([self.interfaces, self.surface_t[:, None]], axis=1)
        return np.max(tc.pi_planck(LD, self.nu[None, None, :], temperatures[:, :, None]), axis=1)

    def isothermal(self):
        """The thermal_cases.Inputs of the same problem: what lbl_path_thermal_two_stream takes."""
        return tc.Inputs(self.name, self.nu, self.beta, self.table, self.surface_t,
                         self.emissivity, self.diffusivity)


def mirror(kind, inputs, from_last):
    """thermal_cases.mirror's dict for the linear-in-tau source."""
    order = inputs.order(from_last).T                               # [L, PATHS]
    eps = inputs.emissivity[:, None] if inputs.emissivity.ndim == 1 else inputs.emissivity
    # With the surface behind level 0 the space-side interface of a level is its last-level side.
    space = 1 if from_last else 0
    edges = inputs.edges[order]                                     # [L, PATHS, 2]
    nu = inputs.nu[None, None, :]
    bt = tc.pi_planck(kind, nu, edges[:, :, space, None])
    bb = tc.pi_planck(kind, nu, edges[:, :, 1 - space, None])
    surface_b = tc.pi_planck(kind, inputs.nu[None, :], inputs.surface_t[:, None])
    li = inputs.layer_inputs(from_last)
    result = adding(kind, tc.layer(kind, li), weight(kind, li), bt, bb, eps, surface_b)
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


per_level = tc.per_level


def worst_error(inputs, from_last):
    """thermal_cases.worst_error for this mirror."""
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
# The first-face Planck alone (1), the carry (2, 3), which are also every loop of path_levels with
# the one row in flight of both kernels (1, A, A + 1, 2A and 2A + 1), and the depths around
# tests/thermal_cases.py's batches of eight.
DEPTHS = (1, 2, 3, 8, 9, 17)
EQUAL_T = 260.


def interfaces_for(table, levels_per_path, seed):
    """Interface temperatures [PATHS, L + 1] and the level table that goes with them: path 0
    random from 150 to 320 K (inversions, dB < 0, among them), path 1 jumping by 30 K from each
    interface to the next, up and down in turn, path 2 with every interface and level at EQUAL_T."""
    rng = np.random.default_rng(seed + 3000)
    interfaces = rng.uniform(150., 320., size=(PATHS, levels_per_path + 1))
    interfaces[1] = 255. + 30.*(np.arange(levels_per_path + 1) % 2)
    interfaces[2] = EQUAL_T
    table = np.array(table, dtype=F64)
    table[2*levels_per_path:, 4] = EQUAL_T
    return interfaces, table


def with_interfaces(inputs, seed):
    interfaces, table = interfaces_for(inputs.table, inputs.levels_per_path, seed)
    out = Inputs(inputs.name, inputs.nu, inputs.beta, table, interfaces, inputs.surface_t,
                 inputs.emissivity, inputs.diffusivity)
    for name in ("cloudy", "group", "omega_c"):
        if hasattr(inputs, name):
            setattr(out, name, getattr(inputs, name))
    return out


def shape_inputs(columns, depth, seed, emissivity_rows=False):
    """thermal_cases.shape_inputs (nu from 0, beta with zeros, a thickness of 0, cloudy and clear
    levels alternating, three surface temperatures none of which is an interface's) with
    interfaces_for's temperatures."""
    return with_interfaces(tc.shape_inputs(columns, depth, seed, emissivity_rows), seed)


CLOUD_PLACES = tc.CLOUD_PLACES + ("none",)


def cloud(place, diffusivity=tc.DIFFUSIVITY):
    """thermal_cases.cloud (clouds at the first, the last or every level of 9: omega_c = 1 over
    beta = 0, beta either side of the conservative threshold, s*beta = 3000, random beta) with
    interfaces_for's temperatures; "none": the table of "first" without its scatterers, and
    s*beta = 1e3 in each path's first and last level in the columns of group 2."""
    base = tc.cloud("first" if place == "none" else place, diffusivity)
    if place == "none":
        base.table[:, 1:4] = 0.
        base.cloudy = np.zeros(base.levels, dtype=bool)
        base.omega_c = np.zeros(base.levels)
        n = base.levels_per_path
        for p in range(PATHS):
            for level in (n*p, n*p + n - 1):
                base.beta[level, base.group == 2] = 1e3/base.table[level, 0]
        base.name = "no cloud"
    return with_interfaces(base, 50 + CLOUD_PLACES.index(place))


def crossing():
    """Every level a cloud of omega_c = 0.9, g_c = 0.5 and tau_c = 0.2 over s*beta rising from 0
    to 3 along 96 columns: y = k*t crosses Y0 inside each wavefront's 64 lanes, at a different
    column in every level (thicknesses from 0.6 to 1.4)."""
    n, columns = 3, 96
    levels = PATHS*n
    thickness = np.linspace(0.6, 1.4, levels)
    tau_c = np.full(levels, 0.2)
    table = np.stack([thickness, tau_c, 0.9*tau_c, np.full(levels, 0.5),
                      np.linspace(200., 300., levels)], axis=1)
    beta = np.broadcast_to(np.linspace(0., 3., columns), (levels, columns)).copy()
    inputs = tc.Inputs("y across y0", np.linspace(50., 2500., columns), beta, table,
                       (250., 288., 320.), tc.EMISSIVITY)
    return with_interfaces(inputs, 60)


def value_cases():
    return [cloud(place) for place in CLOUD_PLACES] + \
        [cloud("every", 2.), cloud("none", 2.), crossing()]


def shape_cases():
    """Every problem the shape tests run: [(inputs, from_last)]."""
    out = []
    for columns in cases.LAYOUT_COLUMNS:
        out.append((shape_inputs(columns, 9, columns), True))
    for depth in DEPTHS:
        for from_last in (False, True):
            out.append((shape_inputs(257, depth, 40 + depth, emissivity_rows=True), from_last))
            out.append((shape_inputs(131, depth, 80 + depth), from_last))
    for _, columns, _ in cases.BAND_SETS:
        out.append((shape_inputs(columns, 3, 70), True))
    return out


def all_cases():
    return shape_cases() + [(inputs, from_last) for inputs in value_cases()
                            for from_last in (False, True)]


def weight_samples(count=200000, seed=11):
    """(k, t, su, g1) of the q scan: y = k*t log-uniform from 1e-8 to 50 and su*t from 1e-6 to 1e3
    with su >= k (k*k = dif*su, dif <= su), g1 = (su + dif)/2, and y at Y0 and its
    neighbours."""
    rng = np.random.default_rng(seed)
    y = 10.**rng.uniform(-8., math.log10(50.), size=count)
    y[:3] = Y0, np.nextafter(Y0, 0.), np.nextafter(Y0, 1.)
    sut = np.maximum(10.**rng.uniform(-6., 3., size=count), y)
    su = rng.uniform(0.2, 2., size=count)
    t = sut/su
    k = y/t
    # dif = k*k/su is 2*g1 - su: g1 follows from k and su.
    g1 = (su + (k*k)/su)/2.
    return k, t, su, g1


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class ThermalSourceRecorder(tc.ThermalRecorder):
    """tests/thermal_cases.py's engine with the call of compute_thermal_flux_linear."""
    def path_thermal_two_stream_source(self, beta, columns, grid, n_paths, levels_per_path,
                                       level_begin, level_table, edge_temperature,
                                       surface_temperature, work, **keywords):
        self.edge_tables = getattr(self, "edge_tables", [])
        self.edge_tables.append((int(level_begin), np.array(edge_temperature)))
        self.record("path_thermal_two_stream_source", beta=beta, columns=columns, grid=grid,
                    n_paths=n_paths, levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table),
                    edge_temperature=np.asarray(edge_temperature),
                    surface_temperature=np.asarray(surface_temperature), work=work,
                    **self._described(keywords))


@contextlib.contextmanager
def recorded(directory):
    """surface_cases.recorded with a ThermalSourceRecorder."""
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = ThermalSourceRecorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before
