"""What tests/test_solar_host.py (CPU), tests/test_gpu_solar_shapes.py and tests/test_gpu_solar.py
(GPU) share: the recurrence of lbl_path_solar in numpy (any float type: float64 "in the stated
order", numpy.longdouble as the reference), the fill of lbl_solar_spectrum (the table as
tests/surface_cases.py's interpolation mirror forms it), numpy mirrors of the host and workgroup arithmetic
of csrc/solar.h that decides which code runs, a stand-in engine with the two calls, and the case
tables.  Columns, layouts and run cuts are tests/sweep_cases.py's."""
import contextlib

import numpy as np

from pylbl_amd.paths import SOLAR_SOLID_ANGLE, SOLAR_TEMPERATURE
from tests import surface_cases as surface
from tests import sweep_cases as cases

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
MAX_KNOTS = 1 << 22         # kSolarMaxKnots of csrc/solar.h
LDS_KNOTS = 1024            # kSurfaceMaxKnots: the slice of knots a workgroup stages
BLOCK_COLUMNS = cases.PATH_THREADS*cases.PATH_WIDTH      # columns of one workgroup
TINY = np.finfo(F64).tiny   # the smallest normal double
STEP = 5e-324               # one subnormal step

MU0 = np.array([1., 1e-3, 0.25])        # three paths, three Suns
ALBEDO = np.array([1., 0.3, 0.])


# ---------------------------------------------------------------------------------------------
# The sweep.
def sweep(kind, beta, solar_lengths, view_lengths, levels_per_path, from_last):
    """tau = tau + a*beta and tv = tv + v*beta from 0 in the Sun's order: (tau, tv) after every
    level, [levels, columns] each (tv None without view_lengths)."""
    tau, _ = cases.sweep_tau(kind, beta, np.asarray(solar_lengths), levels_per_path, from_last)
    tv = None
    if view_lengths is not None:
        tv, _ = cases.sweep_tau(kind, beta, np.asarray(view_lengths), levels_per_path, from_last)
    return tau, tv


def incident(kind, mu0, solar):
    """F0 = mu0*S: [PATHS, columns]."""
    return np.asarray(mu0, dtype=F64).astype(kind)[:, None]*np.asarray(solar, F64).astype(kind)


def last_rows(levels_per_path, from_last):
    """The flat level each path's sweep ends on: the one that touches the surface."""
    return cases._flat(levels_per_path, 0 if from_last else levels_per_path - 1)


def path_of_level(levels_per_path):
    return np.repeat(np.arange(PATHS), levels_per_path)


def direct(kind, f0, tau, levels_per_path):
    """F0*exp(-tau) below every level, [levels, columns], in `kind` from the float64 F0 and tau."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(f0).astype(kind)[path_of_level(levels_per_path)] * \
            np.exp(-np.asarray(tau).astype(kind))


def reflected(kind, f0, albedo, tau, tv, levels_per_path, from_last):
    """((A*F0)/pi)*exp(-(tau + tv)) per path: the quotient and the sum of the two optical depths
    in float64 as written, the exponential and the last product in `kind`.  albedo: [PATHS] or
    [PATHS, columns]."""
    albedo = np.asarray(albedo, dtype=F64)
    if albedo.ndim == 1:
        albedo = albedo[:, None]
    rows = last_rows(levels_per_path, from_last)
    lead = (albedo*np.asarray(f0, dtype=F64))/cases.FLUX_PI
    depth = np.asarray(tau, dtype=F64)[rows] + np.asarray(tv, dtype=F64)[rows]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return lead.astype(kind)*np.exp(-depth.astype(kind))


def mirror(kind, problem, mu0, solar, solar_lengths, from_last, view_lengths=None, albedo=None):
    """The whole recurrence in one float type: {"f0", "tau", "tv", "direct", "reflected"}."""
    n = problem.levels_per_path
    tau, tv = sweep(kind, problem.beta, solar_lengths, view_lengths, n, from_last)
    f0 = incident(kind, mu0, solar)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        out = {"f0": f0, "tau": tau, "tv": tv, "direct": f0[path_of_level(n)]*np.exp(-tau)}
        if view_lengths is not None:
            a = np.asarray(albedo, dtype=F64).astype(kind)
            a = a[:, None] if a.ndim == 1 else a
            rows = last_rows(n, from_last)
            out["reflected"] = ((a*f0)/kind(cases.FLUX_PI))*np.exp(-(tau[rows] + tv[rows]))
    return out


# ---------------------------------------------------------------------------------------------
# The fill.
def interval(knots, nu):
    """surface_cases.interval -- the number of knots <= nu, less one, and -1 for nu <= k_0 and for
    NaN -- by a search, for tables of 2^17 knots (tests/test_solar_host.py compares the two)."""
    knots, nu = np.asarray(knots), np.asarray(nu)
    return np.where(nu > knots[0], np.searchsorted(knots, nu, side="right") - 1, -1)


def table(kind, knots, values, nu, scale=1.):
    """scale*E, E the table at nu as lbl_surface_emissivity interpolates, every operation in `kind`
    and rounded as written: E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j)) for
    k_j <= nu < k_{j+1}, e_0 for nu <= k_0, e_{M-1} for nu >= k_{M-1}."""
    k = np.asarray(knots, dtype=F64).astype(kind)
    e = np.asarray(values, dtype=F64).astype(kind)
    x = np.asarray(nu, dtype=F64).astype(kind)
    last = k.size - 1
    j = interval(k, x)
    inner = np.clip(j, 0, last - 1)
    with np.errstate(over="ignore", invalid="ignore"):
        inside = e[inner] + (x - k[inner])*((e[inner + 1] - e[inner])/(k[inner + 1] - k[inner]))
    return kind(scale)*np.where(j < 0, e[0], np.where(j >= last, e[last], inside))


def blackbody(kind, nu, scale=SOLAR_SOLID_ANGLE, temperature=SOLAR_TEMPERATURE):
    return kind(scale)*cases.planck(kind, nu, kind(temperature))


def fill_routes(knots, nu, ascending=None):
    """Which route each workgroup of solar_spectrum_kernel takes for a table: "staged" (the knots
    between its first and its last column fit LDS) or "searched" (each lane searches in HBM)."""
    knots, nu = np.asarray(knots), np.asarray(nu)
    if ascending is None:
        ascending = bool(np.all(np.diff(nu) >= 0.))
    routes = []
    for first in range(0, nu.size, BLOCK_COLUMNS):
        if not ascending:
            routes.append("searched")
            continue
        end = min(first + BLOCK_COLUMNS, nu.size)
        lo, hi = (int(interval(knots, nu[[j]])[0]) for j in (first, end - 1))
        count = min(hi + 1, knots.size - 1) - max(lo, 0) + 1
        routes.append("staged" if 1 <= count <= LDS_KNOTS else "searched")
    return routes


# name: (knots, grid): the tables and grids of the fill tests.
def fill_cases():
    rng = np.random.default_rng(31)
    grid = np.sort(rng.uniform(2000., 2100., 1300))
    grid[:2] = 2000.                                     # equal points are ascending too
    assert np.all(np.diff(grid) >= 0.)
    out = {}
    for m in (2, 1024, 1025, 1 << 17):
        knots = np.sort(rng.uniform(1990., 2110., m))
        knots[0], knots[-1] = 1990., 2110.
        assert np.all(np.diff(knots) > 0.)
        out["%d knots" % m] = (knots, grid)
    out["grid below the knots"] = (np.linspace(3000., 3100., 50), grid)
    out["grid above the knots"] = (np.linspace(100., 200., 50), grid)
    knots = np.linspace(1995., 2105., 700)
    on = np.concatenate([knots[100:400], np.nextafter(knots[100:400], np.inf),
                         np.nextafter(knots[100:400], -np.inf), [knots[0], knots[-1]]])
    out["grid points on knots"] = (knots, np.sort(on))
    # 5000 knots under the 512 columns of the first workgroup, few under the others.
    dense = np.concatenate([np.linspace(2000., 2030., 5000), np.linspace(2031., 2110., 40)])
    out["slice beyond LDS"] = (dense, grid)
    out["descending grid"] = (out["1025 knots"][0], grid[::-1].copy())
    out["shuffled grid"] = (out["1025 knots"][0], rng.permutation(grid))
    return out


def table_values(knots, seed=5):
    """Irradiances >= 0 at the knots, with zeros among them."""
    values = np.random.default_rng(seed).uniform(0., 3., size=np.asarray(knots).size)
    values[::7] = 0.
    return values


# ---------------------------------------------------------------------------------------------
# The sweep's case tables.
DEPTHS = (1, 8, 9, 16, 17)              # kPathAhead = 8 rows in flight: every loop of path_levels
RUN_DEPTH = 19                          # sweep_cases.run_sets' families need 2*8 + 3 levels


def lengths_of(problem, mu0=MU0):
    """(solar slant lengths thickness/mu0 in float64 as the host forms them, view lengths)."""
    n = problem.levels_per_path
    rng = np.random.default_rng(problem.levels + 1)
    view = rng.uniform(0.5, 2.5, size=problem.levels)
    view[2 % problem.levels] = 0.
    return problem.thickness/np.repeat(np.asarray(mu0, dtype=F64), n), view


def solar_row(problem, seed=3):
    """S on the problem's grid, in [0, 1] (the Sun's is below 1 W m-2 (cm-1)-1 everywhere), with
    columns that are exactly 0."""
    s = np.random.default_rng(seed).uniform(0.05, 1., size=problem.columns)
    s[::5] = 0.
    return s


def value_problem():
    """Values chosen for the arithmetic: sweep_cases.value_problem's beta (groups of columns: all
    zeros, s*beta >= 800 at both ends of every path, mixed sign, random) under mu0 = 1, 1e-3 and
    0.5, albedos 0, 1 and 0.3, and S = 0 in every fifth column."""
    problem = cases.value_problem()
    problem.mu0 = np.array([1., 1e-3, 0.5])
    problem.albedo = np.array([0., 1., 0.3])
    # The slant lengths are given, as solar_path_length allows: a low Sun over mixed signs would
    # only overflow exp in every float type.
    problem.solar_lengths = problem.thickness/np.repeat([1., 0.5, 0.5], problem.levels_per_path)
    _, problem.view_lengths = lengths_of(problem)
    problem.solar = solar_row(problem)
    return problem


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class SolarRecorder(surface.SurfaceRecorder):
    """tests/surface_cases.py's engine with the two solar calls."""
    def _described(self, keywords):
        return {name: (np.asarray(value) if isinstance(value, (list, tuple, np.ndarray))
                       else value) for name, value in sorted(keywords.items())}

    def solar_spectrum(self, grid, row, columns, **keywords):
        self.record("solar_spectrum", grid=grid, row=row, columns=columns,
                    **self._described(keywords))

    def path_solar(self, beta, columns, n_paths, levels_per_path, level_begin, solar_lengths,
                   solar_zenith_cosine, solar_row, carry, **keywords):
        self.record("path_solar", beta=beta, columns=columns, n_paths=n_paths,
                    levels_per_path=levels_per_path, level_begin=level_begin,
                    solar_lengths=np.asarray(solar_lengths),
                    solar_zenith_cosine=np.asarray(solar_zenith_cosine), solar_row=solar_row,
                    carry=carry, **self._described(keywords))


@contextlib.contextmanager
def recorded(directory):
    """surface_cases.recorded with a SolarRecorder."""
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = SolarRecorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before
