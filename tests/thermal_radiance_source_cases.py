"""What tests/test_thermal_radiance_source_host.py (CPU),
tests/test_gpu_thermal_radiance_source_shapes.py and tests/test_gpu_thermal_radiance_linear.py (GPU)
share: the definition of Spectroscopy.compute_thermal_radiance_linear in numpy -- the level of
csrc/thermal_radiance_source.h, for any float type: float64 "as written", numpy.longdouble as the
reference -- a stand-in engine with the call, and the case tables.  The level scalars and the
closed forms of C are tests/thermal_radiance_cases.py's, the problems with their interface
temperatures and the two-stream fluxes of the linear source tests/thermal_source_cases.py's.

Like those mirrors this one continues from the float64 layer inputs (t, w, gp) and the float64
branch decisions: clear, conservative or general, the side of y = 0 and the branch of
linear_weight.  The flux rows are inputs of the kernel: both float types read the same float64
rows, the float64 mirror of thermal_source_cases.  The long-double weight of the thermal term is
tests/linear_source_cases.py's 24-term reference.

scale[p, j] = max B(nu_j, T) over the interface temperatures of path p and its T_s, in long
double: every bound is a multiple of it.

E_CPU is the worst |float64 mirror - long-double mirror|/scale over every case table of this file,
as tests/test_thermal_radiance_source_host.py measures it; the GPU tests hold every radiance to
(4*E_CPU + FLOOR)*scale of the long-double mirror."""
import contextlib

import numpy as np

from tests import linear_source_cases as ls
from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_source_cases as sc

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
VIEW_AHEAD = 1              # kThermalViewSourceAhead
MU = rc.MU
# The worst error of the float64 mirror over the case tables, relative to scale (see above):
# tests/test_thermal_radiance_source_host.py measures 8.78e-10, on the 30 K jumps of path 1 in a
# thin cloud (t = 8e-4) with w = 1 to nine digits, just on the general side of the conservative
# threshold, viewed along mu = 0.6.  Section 27's mirror has its worst in the same branch
# (1.9e-11): P and Q are divided by n = 1 - (Gamma*E)*(Gamma*E), 3e-4 there.  Here u1 and d0 carry -+c with
# c = (pi*dB)/(su*t), which is about 1e3*pi*dB in that level, so that the roundings of P and Q are
# roundings of c/n; they enter the radiance through h and its partner, both about t/mu.  Over the
# cloud tables, which hold the same kind of level, the worst is 4.3e-10; the pole, deep, no-cloud
# and y-across-1/2 tables reach 2e-15.  No cap is set beside it: the figure is what the lines of
# the definition give in float64 and is recorded as measured.
E_CPU = 9e-10
FLOOR = 1e-13
# Bounds of the mirror's properties (tests/test_thermal_radiance_source_host.py), each beside what
# was measured there.
# |C - quadrature|/(|u1| + |d0| + |c|), long double.  Section 27's bound for its two closed forms
# is 9e-17 (measured 4.6e-17); the new term (2*(a*c))*Em is one more closed form of three
# roundings, 3*2^-64 = 1.6e-19 of |c|: the bound stays section 27's.  Measured 4.26e-17; the
# thermal term Bt*Em + dB*(Em - lw) against the quadrature of B(tau), relative to Bt + Bb, is held
# to the same: measured 2.57e-17.
QUADRATURE_BOUND = rc.QUADRATURE_BOUND
# |P*E + Gamma*Q + c - (up[i] - pi*Bt)|/(pi*scale + |c|), long double on long-double fluxes:
# section 27's bounds of its own two branches, for the same reasons (rounding in the general
# branch; what the k = 0 layer leaves out in the conservative one, which its criterion bounds at
# 1e-10), relative to the size of what u1 and d0 hold here: they carry -+c, up to 1e3*pi*scale in
# a thin level under a 30 K jump.  Measured 4.93e-15 and 5.87e-12.
TOP_BOUND = rc.TOP_BOUND
TOP_BOUND_CONSERVATIVE = rc.TOP_BOUND_CONSERVATIVE
# Two halves with the mid-face Planck value on the same line in tau make the level, in
# E_CPU*scale: the fraction of its own E_cpu that section 27 allows its mirror (1.2e-4; it
# measured 6.05e-5), both being roundings of the same lines on the same random levels, whose
# faces here differ by up to 140 K.  Measured 1.18e-5.
SPLIT_BOUND = rc.SPLIT_BOUND

# The lines every statement of the definition holds beside thermal_radiance_cases.FORMULAS' level
# (the header, the docstring of compute_thermal_radiance_linear, DESIGN section 31 and the head of
# csrc/thermal_radiance_source.h).
FORMULAS = (
    "dB = Bb - Bt",
    "c = (pi*dB)/(su*t)",
    "u1 = (up[i+1] - pi*Bb) - c ; d0 = (down[i] - pi*Bt) + c",
    "+ (2*(a*c))*Em",
    "I_top = I_bot*Dm + (Bt*Em + dB*(Em - linear_weight(t/mu, Em))) + (w/(2 pi))*C",
    "x = tau/mu ; A = -expm1(-x) ; lw = linear_weight(x, A)",
    "I_top = I_bot*exp(-x) + (Bb*(A - lw) + Bt*lw)",
)


# ---------------------------------------------------------------------------------------------
# The level.
def source_shift(kind, inputs, bt, bb):
    """c = (pi*dB)/(su*t) of a cloudy level in `kind` (anything in a clear one), and dB."""
    g1, g2, _, _ = rc.scalars(kind, inputs)
    pi = kind(cases.FLUX_PI)
    with np.errstate(all="ignore"):
        db = bb - bt
        return (pi*db)/((g1 + g2)*inputs["t"].astype(kind)), db


def level(kind, inputs, mu, bt, bb, up1, down0, rad):
    """I at the space-side face of one level from `rad` at its surface-side face, in `kind`:
    inputs: layer_inputs of the level's elements; mu broadcastable to them; bt, bb: B at the
    level's space-side and surface-side interfaces in `kind`; up1, down0: the float64 fluxes at
    the level's surface-side and space-side interfaces."""
    two, three = kind(2.), kind(3.)
    pi = kind(cases.FLUX_PI)
    branch = inputs["branch"]
    t = inputs["t"].astype(kind)
    mu64 = np.asarray(mu, dtype=F64)
    mu = mu64.astype(kind)
    positive, series, _ = rc.decisions(inputs, mu64)
    g1, g2, k, w = rc.scalars(kind, inputs)
    with np.errstate(all="ignore"):
        # Clear: t is tau itself; radiance.h's linear_update.
        x = t/mu
        dm = np.exp(-x)
        em = -np.expm1(-x)
        lw = ls.device_weight(x) if kind is F64 else ls.weight(kind, x)
        clear = rad*dm + (bb*(em - lw) + bt*lw)
        # Cloudy.
        a = (three*(inputs["gp"].astype(kind)*mu))/two
        shift, db = source_shift(kind, inputs, bt, bb)
        u1 = (np.asarray(up1, dtype=F64).astype(kind) - pi*bb) - shift
        d0 = (np.asarray(down0, dtype=F64).astype(kind) - pi*bt) + shift
        gamma = g2/(g1 + k)
        c_general, _, _, _ = rc.general_c(kind, k, gamma, t, mu, a, u1, d0, positive)
        c_conservative, _ = rc.conservative_c(kind, g1, t, mu, a, u1, d0, series)
        c = np.where(branch == tc.CONSERVATIVE_BRANCH, c_conservative, c_general)
        c = c + (two*(a*shift))*em
        cloudy = rad*dm + (bt*em + db*(em - lw)) + (w/(two*pi))*c
    return np.where(branch == tc.CLEAR, clear, cloudy)


def flux_rows(inputs, from_last):
    """The float64 flux rows lbl_path_thermal_two_stream_source writes for the problem: {"up",
    "down"} [levels, columns] at the interface below each flat level."""
    fluxes = sc.mirror(F64, inputs, from_last)
    return {q: np.ascontiguousarray(fluxes[q], dtype=F64) for q in tc.QUANTITIES}


def scale(inputs):
    """[PATHS, columns] in long double: max B over the path's interface temperatures and T_s."""
    temperatures = np.concatenate([inputs.interfaces, inputs.surface_t[:, None]], axis=1)
    return np.max(cases.planck(LD, inputs.nu[None, None, :], temperatures[:, :, None]), axis=1)


def face_planck(kind, inputs, rows, side):
    """B in `kind` [PATHS, columns] at side `side` of the flat levels `rows` [PATHS]."""
    return cases.planck(kind, inputs.nu[None, :], inputs.edges[rows, side].astype(kind)[:, None])


def mirror(kind, inputs, mu, from_last, fluxes=None):
    """{"radiance", "brightness_temperature": [PATHS, columns] in `kind`, "scale" in long double}
    of lbl_path_thermal_radiance_source on a thermal_source_cases.Inputs with the view cosines mu
    [PATHS]; fluxes: flux_rows' (None: formed here)."""
    if fluxes is None:
        fluxes = flux_rows(inputs, from_last)
    mu = np.asarray(mu, dtype=F64)
    order = inputs.order(from_last)                             # [PATHS, L], space -> surface
    li = inputs.layer_inputs(from_last)                         # [L, PATHS, columns]
    depth = inputs.levels_per_path
    # With the surface behind level 0 the space-side interface of a level is its last-level side.
    space = 1 if from_last else 0
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
        bt = face_planck(kind, inputs, order[:, i], space)
        bb = face_planck(kind, inputs, order[:, i], 1 - space)
        down0 = fluxes["down"][order[:, i - 1]] if i > 0 else np.zeros_like(fluxes["down"][:PATHS])
        rad = level(kind, here, mu[:, None], bt, bb, fluxes["up"][order[:, i]], down0, rad)
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
# The case tables: section 27's problems (the shapes, the clouds, the pole of h, the deep clouds)
# with section 25's temperatures (thermal_source_cases.interfaces_for: path 0 random with
# inversions, path 1 jumping by 30 K per level, path 2 one temperature throughout; every T_s apart
# from the surface interface's).
def with_view(inputs, seed):
    """thermal_source_cases.with_interfaces, keeping what thermal_radiance_cases' tables carry."""
    out = sc.with_interfaces(inputs, seed)
    for name in ("k", "mu"):
        if hasattr(inputs, name):
            setattr(out, name, getattr(inputs, name))
    return out


def pole():
    return with_view(rc.pole(), 90)


def deep():
    return with_view(rc.deep(), 91)


def shape_inputs(columns, depth, seed, emissivity_rows=False):
    return sc.shape_inputs(columns, depth, seed, emissivity_rows)


def value_cases():
    """[(inputs, mu)]: thermal_source_cases' clouds (at the first level, the last, every level and
    nowhere; y = k*t across Y0) under MU, and section 27's pole and deep tables."""
    out = [(inputs, np.array(MU)) for inputs in sc.value_cases()]
    out.append((with_view(tc.cloud("every", 1.), 92), np.array(MU)))
    for inputs in (pole(), deep()):
        out.append((inputs, inputs.mu))
    return out


def shape_cases():
    """[(inputs, mu, from_last)]: thermal_cases' shape problems with interfaces, under MU."""
    return [(with_view(inputs, 7 + index), np.array(MU), from_last)
            for index, (inputs, from_last) in enumerate(tc.shape_cases())]


def all_cases():
    return shape_cases() + [(inputs, mu, from_last) for inputs, mu in value_cases()
                            for from_last in (False, True)]


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class RadianceSourceRecorder(rc.RadianceRecorder, sc.ThermalSourceRecorder):
    """The engine of both with the call of compute_thermal_radiance_linear."""
    def path_thermal_radiance_source(self, beta, columns, grid, n_paths, levels_per_path,
                                     level_begin, level_table, edge_temperature, view_cosine,
                                     surface_temperature, **keywords):
        self.view_edge_tables = getattr(self, "view_edge_tables", [])
        self.view_edge_tables.append((int(level_begin), np.array(edge_temperature)))
        self.record("path_thermal_radiance_source", beta=beta, columns=columns, grid=grid,
                    n_paths=n_paths, levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table),
                    edge_temperature=np.asarray(edge_temperature),
                    view_cosine=np.asarray(view_cosine),
                    surface_temperature=np.asarray(surface_temperature),
                    **self._described(keywords))


@contextlib.contextmanager
def recorded(directory):
    """surface_cases.recorded with a RadianceSourceRecorder."""
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = RadianceSourceRecorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before
