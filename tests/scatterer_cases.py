"""What tests/test_scatterer_host.py (CPU), tests/test_gpu_scatterer_shapes.py and
tests/test_gpu_scatterer.py (GPU) share: the definition of the spectral scatterer of
include/lbl_amd_scatterer.h in numpy -- where a grid point lies among the knots, the interpolation
and its limit, in float64 as the kernels form them -- handed to the layers and adding recurrences
of tests/two_stream_cases.py, tests/thermal_cases.py and tests/thermal_source_cases.py as the
per-element level table they accept; a stand-in engine with the two calls; and the case tables.
Nothing of the layers is written again here.

    j = the largest index with k_j <= nu, limited to 0 .. M-2
    u = (nu - k_j)/(k_{j+1} - k_j), limited to [0, 1]
    v = e_j + u*(e_{j+1} - e_j), then limited to [min(e_j, e_{j+1}), max(e_j, e_{j+1})]
    w_c = omega_c*tau_c ; h_c = w_c*g_c
A longwave level whose knots all have omega_c*tau_c == 0 is clear (w_c = 0 at every grid point).

E_CPU_SHORTWAVE and E_CPU_LONGWAVE are the worst |float64 mirror - long-double mirror| over every
case table of this file, relative to F0 and to thermal_cases' scale, as
tests/test_scatterer_host.py measures them; the GPU tests hold every flux to
(4*E_CPU + FLUX_FLOOR)*scale of the long-double mirror."""
import contextlib

import numpy as np

from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_source_cases as tsc
from tests import two_stream_cases as ts

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
MAX_KNOTS = 1024            # kScattererMaxKnots
# The method of Spectroscopy that takes the spectral scatterer in place of each grey one's (the
# longwave one serves both sources: interface_temperature selects the linear one).
SPECTRAL_METHOD = {"compute_solar_flux": "compute_solar_flux_spectral",
                   "compute_thermal_flux": "compute_thermal_flux_spectral",
                   "compute_thermal_flux_linear": "compute_thermal_flux_spectral"}
SHORTWAVE_UP_AHEAD = 4      # kTwoStreamSpectralUpAhead
LONGWAVE_UP_AHEAD = 2       # kThermalSpectralUpAhead
# The worst errors of the float64 mirrors over the case tables (see above):
# tests/test_scatterer_host.py measures 1.03e-11 (shortwave; two_stream_cases' own tables, whose
# Suns at mu0 = 1e-3 these share, reach 1.61e-11) and 2.69e-15 (longwave, with either source).
E_CPU_SHORTWAVE = 1.1e-11
E_CPU_LONGWAVE = 3e-15
E_CPU_CAP = 1e-10           # two_stream_cases.E_CPU_CAP and thermal_cases.E_CPU_CAP
FLUX_FLOOR = 1e-13


# ---------------------------------------------------------------------------------------------
# The definition.
def place(knots, nu):
    """(j, u) of every grid point among the knots, in float64."""
    knots, nu = np.asarray(knots, dtype=F64), np.asarray(nu, dtype=F64)
    j = np.clip(np.searchsorted(knots, nu, side="right") - 1, 0, knots.size - 2)
    with np.errstate(all="ignore"):
        u = (nu - knots[j])/(knots[j + 1] - knots[j])
    return j, np.minimum(np.maximum(u, 0.), 1.)


def interpolate(knots, optics, nu):
    """optics [..., M, 3] (tau_c, omega_c, g_c at the knots) on the grid: [..., columns, 3], each
    operation in float64 and rounded as written."""
    optics = np.asarray(optics, dtype=F64)
    j, u = place(knots, nu)
    e0, e1 = optics[..., j, :], optics[..., j + 1, :]
    v = e0 + u[:, None]*(e1 - e0)
    return np.minimum(np.maximum(v, np.minimum(e0, e1)), np.maximum(e0, e1))


def scatters(optics):
    """[levels]: whether some knot of a level has omega_c*tau_c != 0 (else the longwave entry
    takes the level for a clear one)."""
    optics = np.asarray(optics, dtype=F64)
    return np.any(optics[..., 1]*optics[..., 0] != 0., axis=-1)


def shortwave_table(table, knots, optics, nu):
    """The per-element level table [levels, columns, 5] of two_stream_cases.layer_inputs: s_l and
    c_l of `table` [levels, 5] with tau_c, w_c and h_c of the spectral scatterer."""
    e = interpolate(knots, optics, nu)
    w_c = e[..., 1]*e[..., 0]
    out = np.empty(e.shape[:-1] + (5,))
    out[..., 0], out[..., 1] = table[:, None, 0], table[:, None, 1]
    out[..., 2], out[..., 3], out[..., 4] = e[..., 0], w_c, w_c*e[..., 2]
    return out


def longwave_table(table, knots, optics, nu):
    """The per-element level table [levels, columns, 5] of thermal_cases.layer_inputs: s_l and T_l
    of `table` [levels, 5] with tau_c, w_c and g_c of the spectral scatterer; w_c = 0 in a level
    that does not scatter."""
    e = interpolate(knots, optics, nu)
    out = np.empty(e.shape[:-1] + (5,))
    out[..., 0], out[..., 4] = table[:, None, 0], table[:, None, 4]
    out[..., 1], out[..., 3] = e[..., 0], e[..., 2]
    out[..., 2] = np.where(scatters(optics)[:, None], e[..., 1]*e[..., 0], 0.)
    return out


# ---------------------------------------------------------------------------------------------
# Problems of PATHS paths in flat storage, as the two entries take them: the grey Inputs with the
# scatterer words of the table at 0, the grid, the knots [M] and the optics [levels, M, 3].
class _Spectral(object):
    def spectral(self, nu, knots, optics):
        self.nu = np.ascontiguousarray(nu, dtype=F64)
        self.knots = np.ascontiguousarray(knots, dtype=F64)
        self.optics = np.ascontiguousarray(optics, dtype=F64)
        assert self.optics.shape == (self.levels, self.knots.size, 3)
        assert self.nu.shape == (self.columns,)


class Shortwave(ts.Inputs, _Spectral):
    def __init__(self, name, nu, beta, table, mu0, solar_row, sigma, albedo, knots, optics):
        ts.Inputs.__init__(self, name, beta, table, mu0, solar_row, sigma, albedo)
        self.spectral(nu, knots, optics)
        assert np.all(self.table[:, 2:] == 0.)

    def layer_inputs(self, from_last):
        order = self.sun_order(from_last).T                      # [L, PATHS]
        table = shortwave_table(self.table, self.knots, self.optics, self.nu)
        return ts.layer_inputs(table[order], self.mu0[None, :, None], self.beta[order],
                               self.sigma[None, None, :])

    def grey(self, level_optics):
        """The two_stream_cases.Inputs of the same problem with the grey scatterer level_optics
        [levels, 3] (tau_c, omega_c, g_c)."""
        table = self.table.copy()
        w_c = level_optics[:, 1]*level_optics[:, 0]
        table[:, 2], table[:, 3], table[:, 4] = level_optics[:, 0], w_c, w_c*level_optics[:, 2]
        return ts.Inputs(self.name, self.beta, table, self.mu0, self.solar, self.sigma,
                         self.albedo)


class Longwave(tsc.Inputs, _Spectral):
    """With interface temperatures: tsc.mirror is the linear source's mirror, and tc.mirror of
    isothermal() the one of the level temperatures."""
    def __init__(self, name, nu, beta, table, interfaces, surface_t, emissivity, knots, optics,
                 diffusivity=tc.DIFFUSIVITY):
        tsc.Inputs.__init__(self, name, nu, beta, table, interfaces, surface_t, emissivity,
                            diffusivity)
        self.spectral(nu, knots, optics)
        assert np.all(self.table[:, 1:4] == 0.)

    def layer_inputs(self, from_last):
        order = self.order(from_last).T                          # [L, PATHS]
        table = longwave_table(self.table, self.knots, self.optics, self.nu)
        return tc.layer_inputs(table[order], self.diffusivity, self.beta[order])

    def isothermal(self):
        return Isothermal(self)

    def grey(self, level_optics):
        """The thermal_source_cases.Inputs of the same problem with the grey scatterer
        level_optics [levels, 3] (tau_c, omega_c, g_c)."""
        table = self.table.copy()
        table[:, 1], table[:, 2] = level_optics[:, 0], level_optics[:, 1]*level_optics[:, 0]
        table[:, 3] = level_optics[:, 2]
        return tsc.Inputs(self.name, self.nu, self.beta, table, self.interfaces, self.surface_t,
                          self.emissivity, self.diffusivity)


class Isothermal(tc.Inputs):
    """A Longwave problem as thermal_cases.mirror takes it: the source of the level temperatures
    (scale: theirs)."""
    def __init__(self, spectral):
        tc.Inputs.__init__(self, spectral.name, spectral.nu, spectral.beta, spectral.table,
                           spectral.surface_t, spectral.emissivity, spectral.diffusivity)
        self.layer_inputs = spectral.layer_inputs


def shortwave_mirror(kind, inputs, from_last):
    """two_stream_cases.mirror's dict with the spectral scatterer."""
    return ts.mirror(kind, inputs, from_last)


def longwave_mirror(kind, inputs, from_last, linear):
    """thermal_source_cases.mirror's (linear) or thermal_cases.mirror's dict with the spectral
    scatterer."""
    if linear:
        return tsc.mirror(kind, inputs, from_last)
    return tc.mirror(kind, inputs.isothermal(), from_last)


def longwave_worst_error(inputs, from_last, linear):
    if linear:
        return tsc.worst_error(inputs, from_last)
    return tc.worst_error(inputs.isothermal(), from_last)


# ---------------------------------------------------------------------------------------------
# The knots.
def knots_for(nu, m, seed=0):
    """M knots for a grid `nu` [columns] in any order.  With at least 8 columns: one knot between
    the two columns of a lane (columns 2a and 2a + 1), one between two lanes of a wavefront
    (columns 2b + 1 and 2b + 2) and one exactly on a grid point, with grid points below k_0 and
    above k_{M-1}; M = 2 takes the first two, larger M adds random knots between the outermost of
    the three and a sixteenth of the grid beyond them.  With fewer columns: the middle grid point
    is k_0, and the last knot lies below the next grid point."""
    nu = np.sort(np.asarray(nu, dtype=F64))
    n = nu.size
    if n < 8:
        above = nu[n//2 + 1] - nu[n//2] if n//2 + 1 < n else 2.
        return nu[n//2] + np.linspace(0., 0.5*above, m)
    a, b, c = n//8, n//4, (3*n)//4
    b += 1 if b % 64 == 63 else 0
    special = [0.5*(nu[2*a] + nu[2*a + 1]), 0.5*(nu[2*b + 1] + nu[2*b + 2]), nu[c]]
    if m == 2:
        return np.array(special[:2])
    rng = np.random.default_rng(900 + seed)
    low, high = nu[max(1, 2*a - n//16)], nu[min(n - 2, c + n//16)]
    knots = np.sort(np.concatenate([special, rng.uniform(low, high, size=m - 3)]))
    assert np.all(np.diff(knots) > 0.) and nu[0] < knots[0] and knots[-1] < nu[-1]
    return knots


# What the scatterer of a level is, in turn from level to level (offset by the path): none at all,
# one that only absorbs, one that scatters at some knots only, a random one with omega_c in {0, 1}
# among random values and g_c up to 0.9, and one whose tau_c falls to exactly 0 at a knot.
KINDS = ("none", "absorbing", "some knots", "random", "to zero")


def optics_for(levels, levels_per_path, m, seed, g_max=0.9):
    """(optics [levels, M, 3], kind [levels]) with the kinds above."""
    rng = np.random.default_rng(700 + seed)
    index = np.arange(levels)
    kind = (index % levels_per_path + 2*(index//levels_per_path) + 3) % len(KINDS)
    tau = 10.**rng.uniform(-3., 1.5, size=(levels, m))
    omega = rng.choice([0., 1., 0.5, 0.999999], size=(levels, m))
    omega = np.where(omega == 0.5, rng.uniform(0., 1., size=(levels, m)), omega)
    g = rng.choice([0., g_max, 0.5], size=(levels, m))
    g = np.where(g == 0.5, rng.uniform(0., g_max, size=(levels, m)), g)
    knot = np.arange(m)[None, :]
    for k, name in enumerate(KINDS):
        rows = (kind == k)[:, None]
        if name == "none":
            tau = np.where(rows, 0., tau)
        elif name == "absorbing":
            omega = np.where(rows, 0., omega)
        elif name == "some knots":
            # Every other knot scatters (omega_c > 0 there); the ones between only absorb.
            omega = np.where(rows, np.where(knot % 2 == 1, np.maximum(omega, 0.3), 0.), omega)
        elif name == "to zero":
            # tau_c is exactly 0 at every other knot (M = 2 and 3: at the last one).
            omega = np.where(rows, np.maximum(omega, 0.2), omega)
            tau = np.where(rows & (knot % 2 == (m - 1) % 2) & (knot > 0 if m > 2 else knot == 1),
                           0., tau)
    return np.stack([tau, omega, g], axis=2), kind


# ---------------------------------------------------------------------------------------------
# The case tables.
DEPTHS = (1, 8, 9, 17)          # the loops of path_levels with 8, 4, 2 and 1 rows in flight
KNOT_COUNTS = (2, 3, MAX_KNOTS)
# M for each of sweep_cases.LAYOUT_COLUMNS and for each depth.
LAYOUT_KNOTS = dict(zip(cases.LAYOUT_COLUMNS, (3, 2, MAX_KNOTS, 3, MAX_KNOTS)))
DEPTH_KNOTS = dict(zip(DEPTHS, (MAX_KNOTS, 2, 3, MAX_KNOTS)))
DEPTH_COLUMNS = 513


def _grid(problem, descending):
    return problem.nu[::-1].copy() if descending else problem.nu


def shortwave_inputs(columns, depth, m, seed, descending=False, albedo_rows=False):
    """two_stream_cases.shape_inputs' problem (beta with zeros, a thickness of 0, Rayleigh depths
    up to ~1) with a spectral scatterer of M knots in place of the grey one."""
    base = ts.shape_inputs(columns, depth, seed, albedo_rows)
    problem = cases.Problem(columns, depth, seed=seed)
    nu = _grid(problem, descending)
    table = base.table.copy()
    table[:, 2:] = 0.
    optics, kind = optics_for(base.levels, depth, m, seed)
    inputs = Shortwave("shortwave %d x %d, M = %d" % (columns, depth, m), nu, base.beta, table,
                       base.mu0, base.solar, base.sigma, base.albedo, knots_for(nu, m, seed),
                       optics)
    inputs.kind = kind
    return inputs


def longwave_inputs(columns, depth, m, seed, descending=False, emissivity_rows=False):
    """thermal_source_cases.shape_inputs' problem (nu from 0, beta with zeros, a thickness of 0,
    interface temperatures with inversions, jumps and an isothermal path) with a spectral
    scatterer of M knots in place of the grey one; g_c up to 0.85 as there."""
    base = tsc.shape_inputs(columns, depth, seed, emissivity_rows)
    nu = base.nu[::-1].copy() if descending else base.nu
    table = base.table.copy()
    table[:, 1:4] = 0.
    optics, kind = optics_for(base.levels, depth, m, seed, g_max=0.85)
    inputs = Longwave("longwave %d x %d, M = %d" % (columns, depth, m), nu, base.beta, table,
                      base.interfaces, base.surface_t, base.emissivity, knots_for(nu, m, seed),
                      optics)
    inputs.kind = kind
    return inputs


def _to_zero(inputs):
    """Moves three neighbouring grid points of `inputs` onto the middle knot of its three and one
    ulp to either side of it, and makes tau_c exactly 0 there in every level that has a scatterer:
    one ulp below, u is the largest double under 1 and the rounded interpolation may leave the
    knots' range, which the limit must not let it do."""
    assert inputs.knots.size == 3 and np.all(np.diff(inputs.nu) > 0.)
    k = inputs.knots[1]
    c = int(np.searchsorted(inputs.nu, k))
    assert 2 <= c < inputs.columns - 2
    inputs.nu[c - 1:c + 2] = np.nextafter(k, -np.inf), k, np.nextafter(k, np.inf)
    assert np.all(np.diff(inputs.nu) > 0.)
    has = np.any(inputs.optics[:, :, 0] > 0., axis=1)
    inputs.optics[:, 0, 0] = np.where(has, np.maximum(inputs.optics[:, 0, 0], 0.7), 0.)
    inputs.optics[:, 2, 0] = np.where(has, np.maximum(inputs.optics[:, 2, 0], 3.), 0.)
    inputs.optics[:, 1, 0] = 0.
    inputs.at_zero = c
    inputs.name += ", tau_c to zero"
    return inputs


def shortwave_to_zero():
    return _to_zero(shortwave_inputs(67, 3, 3, 5))


def longwave_to_zero():
    return _to_zero(longwave_inputs(67, 3, 3, 5))


def _cases(make, rows):
    out = []
    for columns in cases.LAYOUT_COLUMNS:
        out.append((make(columns, 9, LAYOUT_KNOTS[columns], columns), True))
    for depth in DEPTHS:
        for from_last in (False, True):
            out.append((make(DEPTH_COLUMNS, depth, DEPTH_KNOTS[depth], 40 + depth,
                             **{rows: True}), from_last))
    out.append((make(131, 3, 3, 7, descending=True), False))
    out.append((make(130, 8, MAX_KNOTS, 8, descending=True), True))
    return out


def shortwave_cases():
    """Every problem of the shortwave entry: [(inputs, from_last)]."""
    return _cases(shortwave_inputs, "albedo_rows") + \
        [(shortwave_to_zero(), from_last) for from_last in (False, True)]


def longwave_cases():
    """Every problem of the longwave entry, each run with both sources: [(inputs, from_last)]."""
    return _cases(longwave_inputs, "emissivity_rows") + \
        [(longwave_to_zero(), from_last) for from_last in (False, True)]


def flat_optics(level_optics, m):
    """[levels, 3] repeated along a knot axis of M: [levels, M, 3]."""
    return np.ascontiguousarray(np.repeat(np.asarray(level_optics, dtype=F64)[:, None, :], m,
                                          axis=1))


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class ScattererRecorder(tsc.ThermalSourceRecorder):
    """tests/thermal_source_cases.py's engine with the two spectral calls."""
    def path_two_stream_spectral(self, beta, columns, grid, n_paths, levels_per_path, level_begin,
                                 level_table, knot_wavenumber, knot_optics, solar_zenith_cosine,
                                 solar_row, work, **keywords):
        self.knot_tables = getattr(self, "knot_tables", [])
        self.knot_tables.append((int(level_begin), np.array(knot_wavenumber),
                                 np.array(knot_optics)))
        self.record("path_two_stream_spectral", beta=beta, columns=columns, grid=grid,
                    n_paths=n_paths, levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table),
                    knot_wavenumber=np.asarray(knot_wavenumber),
                    knot_optics=np.asarray(knot_optics),
                    solar_zenith_cosine=np.asarray(solar_zenith_cosine), solar_row=solar_row,
                    work=work, **self._described(keywords))

    def path_thermal_two_stream_spectral(self, beta, columns, grid, n_paths, levels_per_path,
                                         level_begin, level_table, knot_wavenumber, knot_optics,
                                         surface_temperature, work, **keywords):
        self.knot_tables = getattr(self, "knot_tables", [])
        self.knot_tables.append((int(level_begin), np.array(knot_wavenumber),
                                 np.array(knot_optics)))
        self.record("path_thermal_two_stream_spectral", beta=beta, columns=columns, grid=grid,
                    n_paths=n_paths, levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table),
                    knot_wavenumber=np.asarray(knot_wavenumber),
                    knot_optics=np.asarray(knot_optics),
                    surface_temperature=np.asarray(surface_temperature), work=work,
                    **self._described(keywords))


@contextlib.contextmanager
def recorded(directory):
    """surface_cases.recorded with a ScattererRecorder."""
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = ScattererRecorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before
