"""What tests/test_thermal_radiance_observer_host.py (CPU),
tests/test_gpu_thermal_radiance_observer_shapes.py and tests/test_gpu_thermal_radiance_observer.py
(GPU) share: the definition of Spectroscopy.compute_thermal_radiance_at in numpy -- the sweep of
csrc/thermal_radiance_observer.h, for any float type: float64 "as written", numpy.longdouble as the
reference --, a stand-in engine with the call, and the case tables.  The levels are
tests/thermal_radiance_cases.py's (isothermal) and tests/thermal_radiance_source_cases.py's (linear
in tau), called with the arguments the definition exchanges; the flux rows are the float64 mirrors
of tests/thermal_cases.py and tests/thermal_source_cases.py.

A problem is linear where it carries interface temperatures (thermal_source_cases.with_interfaces);
otherwise its levels are isothermal.

scale[p, j] is the existing one of each source: max B over the path's temperatures and T_s.

E_CPU (isothermal) and E_CPU_LINEAR are the worst |float64 mirror - long-double mirror|/scale over
every case table, observer and direction of this file, as
tests/test_thermal_radiance_observer_host.py measures them; the GPU tests hold every radiance to
(4*E + FLOOR)*scale of the long-double mirror, E being the one of the problem's source."""
import contextlib

import numpy as np

from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_radiance_source_cases as src

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
VIEW_AHEAD = 1              # kThermalObserverAhead
MU = rc.MU
LOOKING = ("down", "up")
# The worst error of the float64 mirror over thermal_cases' shape and value cases with pole() and
# deep(), every observer below and both directions, relative to scale:
# tests/test_thermal_radiance_observer_host.py measures 2.11e-11 looking down (shape 513 x 8, the
# observer after 7 of its 8 levels: thermal_radiance_cases' worst, 1.9e-11 at the top of the path,
# before the last level attenuates it) and 8.7e-12 looking up.  It stays below the project's cap.
E_CPU = 2.2e-11
E_CPU_CAP = rc.E_CPU_CAP
# The same over thermal_radiance_source_cases' tables, which are those problems with
# thermal_source_cases' interface temperatures: measured 2.02e-9 in both directions, in the middle
# of "cloud at every" (n_p = 4 of 9).  That module measures 8.78e-10 at the top of the same paths,
# made in a thin, nearly conservative cloud under a 30 K jump, where the roundings of P and Q are
# roundings of c/n; an observer inside the atmosphere sees that level's error before the levels
# above attenuate it.  n_p = L looking down is that module's mirror exactly, so no cap below its
# 8.78e-10 can hold here; like that module's, the figure has no cap beside it and is recorded as
# measured.
E_CPU_LINEAR = 2.1e-9
FLOOR = 1e-13
# |C with u1 and d0 exchanged - quadrature of the down-travelling ray|/(|u1| + |d0|), long double:
# measured 4.86e-17, beside thermal_radiance_cases' 4.6e-17 for the same closed forms read the
# other way; with the linear source's shift, over |u1| + |d0| + |c|, 4.64e-17.  The bound is that
# module's, about twice the measured values.  A wrong exchange differs at order 1.
QUADRATURE_BOUND = rc.QUADRATURE_BOUND
# Directly under thermal_cases' opaque lid (a grey absorber of tau_c = 3000 without scattering)
# looking up gives B of the lid's level, relative to scale, float64 mirror: measured 0 --
# exp(-3000/mu) underflows and -expm1(-3000/mu) is 1, so the clear line is 0*I + B*1.
LID_BOUND = 0.

# The lines every statement of the definition holds (the header, the docstring of
# compute_thermal_radiance_at, DESIGN section 32 and the head of csrc/thermal_radiance_observer.h).
FORMULAS = (
    "F_with = up[i+1] ; F_against = down[i]",
    "F_with = down[i] ; F_against = up[i+1]",
    "c = (pi*(B_space - B_surface))/(su*t)",
    "u1 = (down[i] - pi*B_space) - c ; d0 = (up[i+1] - pi*B_surface) + c",
)


def linear(inputs):
    return hasattr(inputs, "edges")


def flux_rows(inputs, from_last):
    """The float64 flux rows of the problem's flux entry: {"up", "down"} [levels, columns]."""
    return (src if linear(inputs) else rc).flux_rows(inputs, from_last)


def scale(inputs):
    return (src if linear(inputs) else rc).scale(inputs)


def surface_line(kind, inputs, from_last, fluxes):
    """The start of a view down, thermal_radiance_cases.mirror's: [PATHS, columns] in `kind`."""
    order = inputs.order(from_last)
    eps = inputs.emissivity[:, None] if inputs.emissivity.ndim == 1 else inputs.emissivity
    eps = np.asarray(eps, dtype=F64).astype(kind)
    one, pi = kind(1.), kind(cases.FLUX_PI)
    with np.errstate(all="ignore"):
        surface_down = fluxes["down"][order[:, -1]].astype(kind)
        return eps*cases.planck(kind, inputs.nu[None, :], inputs.surface_t[:, None]) + \
            (one - eps)*(surface_down/pi)


def through(kind, inputs, li, order, from_last, mu, i, up, fluxes, rad):
    """I_X from I_E = rad through level i (counted from space) of every path, in `kind`: the
    existing levels with F_with, F_against, B_E and B_X in the places of up[i+1], down[i], Bb and
    Bt."""
    here = {name: (value[i] if isinstance(value, np.ndarray) and value.ndim == 3 else value)
            for name, value in li.items()}
    own_up = fluxes["up"][order[:, i]]
    above_down = fluxes["down"][order[:, i - 1]] if i > 0 else \
        np.zeros_like(fluxes["down"][:PATHS])
    f_with, f_against = (above_down, own_up) if up else (own_up, above_down)
    if not linear(inputs):
        b = cases.planck(kind, inputs.nu[None, :], inputs.table[order[:, i], 4][:, None])
        return rc.level(kind, here, mu[:, None], b, f_with, f_against, rad)
    space = 1 if from_last else 0
    b_space = src.face_planck(kind, inputs, order[:, i], space)
    b_surface = src.face_planck(kind, inputs, order[:, i], 1 - space)
    b_enter, b_leave = (b_space, b_surface) if up else (b_surface, b_space)
    return src.level(kind, here, mu[:, None], b_leave, b_enter, f_with, f_against, rad)


def mirror(kind, inputs, mu, from_last, passed, up, fluxes=None, start=None):
    """{"radiance", "brightness_temperature": [PATHS, columns] in `kind`, "scale" in long double}
    of lbl_path_thermal_radiance_observer on the problem with the view cosines mu [PATHS] and
    passed [PATHS]: n_p.  up: looking up.  fluxes: flux_rows' (None: formed here).  start: the
    radiance at the ray's first interface in place of the definition's, with skip = start[1] levels
    already behind it (for the composition property): (radiance, skip)."""
    if fluxes is None:
        fluxes = flux_rows(inputs, from_last)
    mu = np.asarray(mu, dtype=F64)
    passed = np.asarray(passed)
    order = inputs.order(from_last)                             # [PATHS, L], space -> surface
    li = inputs.layer_inputs(from_last)                         # [L, PATHS, columns]
    depth = inputs.levels_per_path
    assert passed.shape == (PATHS,) and np.all((passed >= 0) & (passed <= depth))
    nu = inputs.nu[None, :]
    skip = np.zeros(PATHS, dtype=int)
    if start is not None:
        rad, skip = start[0].astype(kind), np.asarray(start[1])
    elif up:
        rad = np.zeros((PATHS, inputs.columns), dtype=kind)
    else:
        rad = surface_line(kind, inputs, from_last, fluxes)
    for step in range(depth):
        i = step if up else depth - 1 - step
        active = (step >= skip) & (step < passed)
        if not np.any(active):
            continue
        new = through(kind, inputs, li, order, from_last, mu, i, up, fluxes, rad)
        rad = np.where(active[:, None], new, rad)
    return {"radiance": rad, "brightness_temperature": cases.brightness(kind, nu, rad),
            "scale": scale(inputs)}


def worst_error(inputs, mu, from_last, passed, up, fluxes=None):
    """The worst |float64 mirror - long-double mirror|/scale of the radiance (columns with scale =
    0 must agree exactly), and whether everything is finite."""
    if fluxes is None:
        fluxes = flux_rows(inputs, from_last)
    low = mirror(F64, inputs, mu, from_last, passed, up, fluxes)
    high = mirror(LD, inputs, mu, from_last, passed, up, fluxes)
    size = low["scale"]
    finite = bool(np.all(np.isfinite(low["radiance"])) and np.all(np.isfinite(high["radiance"])))
    error = np.abs(low["radiance"].astype(LD) - high["radiance"])
    dark = size == 0.
    assert np.all(error[dark] == 0.)
    worst = float(np.max(error[~dark]/size[~dark])) if np.any(~dark) else 0.
    return worst, finite


# ---------------------------------------------------------------------------------------------
# The observers.
def interfaces(depth):
    """The interfaces (counted from space: the levels a view up passes) an observer is placed at:
    every one for depths <= 3, {0, 1, L//2, L - 1, L} beyond."""
    if depth <= 3:
        return list(range(depth + 1))
    return sorted({0, 1, depth//2, depth - 1, depth})


def observers(depth):
    """[passed [PATHS]]: every n_p of interfaces(depth) for all three paths at once, and one call
    with three different n_p across the paths (two where the depth has only two)."""
    places = interfaces(depth)
    out = [np.full(PATHS, n, dtype=np.int32) for n in places]
    mixed = np.array([places[(1 + p) % len(places)] for p in range(PATHS)], dtype=np.int32)
    out.append(mixed)
    assert len(set(mixed.tolist())) == min(3, len(places))
    return out


# ---------------------------------------------------------------------------------------------
# The case tables: thermal_radiance_cases' (isothermal) and thermal_radiance_source_cases' (the same
# problems with interface temperatures).
def all_cases(source):
    """[(inputs, mu, from_last)] of the source "isothermal" or "linear": the shape and the value
    cases, pole() and deep() among them, the value cases with both surface ends."""
    return (src if source == "linear" else rc).all_cases()


def views(source):
    """Every view of the tables: (inputs, mu, from_last, passed, up)."""
    for inputs, mu, from_last in all_cases(source):
        for passed in observers(inputs.levels_per_path):
            for up in (False, True):
                yield inputs, mu, from_last, passed, up


def pitfall():
    """The smallest problem in which cutting the step count of the existing loop would be wrong: 2
    levels per path, a cloud in the level nearer the surface (the last one: surface behind the last
    level), the observer between the levels, looking down -- the cloud's F_against is the real
    down row at interface 1, not the 0 of the path's space end."""
    rng = np.random.default_rng(5)
    columns, n = 7, 2
    levels = PATHS*n
    index = np.arange(levels)
    lower = index % n == n - 1
    tau_c = np.where(lower, 2., 0.)
    table = np.stack([np.ones(levels), tau_c, 0.9*tau_c, np.where(lower, 0.6, 0.),
                      np.linspace(220., 290., levels)], axis=1)
    beta = 10.**rng.uniform(-2., 0.5, size=(levels, columns))
    return tc.Inputs("pitfall", np.linspace(100., 2000., columns), beta, table, (250., 288., 320.),
                     tc.EMISSIVITY)


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class RadianceObserverRecorder(src.RadianceSourceRecorder):
    """thermal_radiance_source_cases' engine (a RadianceRecorder) with the call of
    compute_thermal_radiance_at."""
    def path_thermal_radiance_observer(self, beta, columns, grid, n_paths, levels_per_path,
                                       level_begin, level_table, view_cosine, observer_levels,
                                       surface_temperature, **keywords):
        self.observer_levels = getattr(self, "observer_levels", [])
        self.observer_levels.append(np.array(observer_levels))
        edges = keywords.pop("edge_temperature")
        if edges is not None:
            keywords["edge_temperature"] = np.asarray(edges)
        self.record("path_thermal_radiance_observer", beta=beta, columns=columns, grid=grid,
                    n_paths=n_paths, levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table), view_cosine=np.asarray(view_cosine),
                    surface_temperature=np.asarray(surface_temperature),
                    **self._described(keywords))


assert issubclass(RadianceObserverRecorder, rc.RadianceRecorder)


@contextlib.contextmanager
def recorded(directory):
    """surface_cases.recorded with a RadianceObserverRecorder."""
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = RadianceObserverRecorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before
