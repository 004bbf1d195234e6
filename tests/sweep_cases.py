"""What tests/test_sweep_host.py (CPU) and tests/test_gpu_sweep_shapes.py (GPU) share: synthetic
inputs for lbl_path_compute, lbl_path_radiance and lbl_path_flux, the three recurrences of
include/lbl_amd.h in numpy (any float type: float64 "in the stated order", numpy.longdouble as the
reference, each with its companion recurrence over magnitudes), numpy mirrors of the host and lane
arithmetic of csrc/path.h, flux.h and path_entry.inc that decides which code runs, and the case
tables both files iterate over."""
from collections import namedtuple

import numpy as np

from pylbl_amd.spectroscopy import PLANCK_C1, PLANCK_C2, flux_angles

# csrc/path.h and csrc/flux.h (tests/test_sweep_host.py reads the headers and compares).
PATH_THREADS = 256      # kPathThreads
PATH_WIDTH = 2          # kPathWidth
PATH_AHEAD = 8          # kPathAhead
PATH_SEGMENT = 4096     # kPathSegment
FLUX_MAX_ANGLES = 8     # kFluxMaxAngles
FLUX_AHEAD_MANY = 4     # kFluxAhead<K> for K > FLUX_AHEAD_SPLIT
FLUX_AHEAD_SPLIT = 4
FLUX_PI = 3.141592653589793     # kFluxPi

LD = np.longdouble
PATHS = 3
SENTINEL = -12345.678


def flux_ahead(angles):
    return PATH_AHEAD if angles <= FLUX_AHEAD_SPLIT else FLUX_AHEAD_MANY


# ---------------------------------------------------------------------------------------------
# Layouts: the row stride for a column count and the offset [values] of every base from a
# 16-byte aligned allocation.
Layout = namedtuple("Layout", "name stride offset")
LAYOUTS = {x.name: x for x in (
    Layout("aligned", lambda columns: columns + columns % 2, 0),    # the vector kernels
    Layout("exact", lambda columns: columns, 0),                    # stride = columns
    Layout("padded", lambda columns: columns + 3, 0),               # NaN in the padding
    Layout("offset", lambda columns: columns + columns % 2, 1),     # even stride, base + 8 bytes
    Layout("odd", lambda columns: columns + 1 - columns % 2, 0),    # odd stride
)}


def path_vector(stride, offsets):
    """path_entry.inc's path_vector: an even stride and every base 16-byte aligned."""
    return stride % 2 == 0 and all(offset % 2 == 0 for offset in offsets)


def layout_is_vector(name, columns):
    layout = LAYOUTS[name]
    return path_vector(layout.stride(columns), [layout.offset])


def lane_widths(columns):
    """The widths of path_lane's lanes that are not idle."""
    return {min(columns - j, PATH_WIDTH) for j in range(0, columns, PATH_WIDTH)}


Lane = namedtuple("Lane", "path n starts finishes")


def path_lanes(first, count, levels_per_path, from_last):
    """path_lane for the launch of the run [first, first + count): one Lane per path touched."""
    lanes = []
    for p in range(first//levels_per_path, (first + count - 1)//levels_per_path + 1):
        path_lo, path_hi = p*levels_per_path, (p + 1)*levels_per_path
        lo, hi = max(first, path_lo), min(first + count, path_hi)
        assert lo < hi
        starts = hi == path_hi if from_last else lo == path_lo
        finishes = lo == path_lo if from_last else hi == path_hi
        lanes.append(Lane(p, hi - lo, starts, finishes))
    return lanes


def batches(n, ahead):
    """path_levels: (full batches of `ahead` rows in flight, remainder steps)."""
    return n//ahead, n % ahead


def depth_class(n, ahead):
    """Which loops of path_levels a lane of n steps runs."""
    full, rest = batches(n, ahead)
    if full == 0:
        return "below"
    if rest == 0:
        return "one batch" if full == 1 else "batches"
    return "batch and remainder" if full == 1 else "batches and remainder"


def band_segments(band_start):
    """PathBands: [(band, begin, end)], every band cut at multiples of PATH_SEGMENT."""
    segments = []
    for b in range(len(band_start) - 1):
        c = int(band_start[b])
        while c < band_start[b + 1]:
            end = min((c//PATH_SEGMENT + 1)*PATH_SEGMENT, int(band_start[b + 1]))
            segments.append((b, c, end))
            c = end
    return segments


# ---------------------------------------------------------------------------------------------
# Runs of flat levels over PATHS paths of L levels, in storage order (a from-last sweep issues
# them reversed).
def runs_from_cuts(cuts):
    cuts = sorted(set(cuts))
    return [(a, b - a) for a, b in zip(cuts, cuts[1:])]


def cuts_of_splits(splits, levels_per_path):
    """Each path cut into the pieces given for it."""
    cuts = {0}
    for p, pieces in enumerate(splits):
        assert sum(pieces) == levels_per_path
        at = p*levels_per_path
        for piece in pieces:
            at += piece
            cuts.add(at)
    return cuts


def run_sets(levels_per_path, ahead=None):
    """{name: runs}.  Always: the whole atmosphere in one call, one level per call, and uneven runs
    whose middle one holds the tail of path 0, all of path 1 and the head of path 2
    ([0, 11), [11, 49), [49, 57) for 3 x 19).  With `ahead` (levels_per_path = 2*ahead + 3): splits
    that give every (starts, finishes) pair a lane below, at, above and beyond twice `ahead`, and
    their mirror images for the other direction."""
    n = levels_per_path
    total = PATHS*n
    sets = {"whole": [(0, total)], "levels": [(i, 1) for i in range(total)]}
    a = (11*n)//19
    uneven = {0, a, 2*n + a, total}
    sets["uneven"] = runs_from_cuts(uneven)
    sets["uneven mirrored"] = runs_from_cuts({total - c for c in uneven})
    if ahead is not None:
        assert n == 2*ahead + 3
        families = {
            "deep": [(1, 2*ahead + 1, 1), (ahead, ahead, 3), (ahead + 1, ahead + 1, 1)],
            "ends": [(2*ahead + 1, 1, 1), (1, 1, 2*ahead + 1), (2, ahead, ahead + 1)],
            "thirds": [(3, ahead, ahead), (ahead, 3, ahead), (ahead, ahead, 3)],
        }
        for name, splits in families.items():
            cuts = cuts_of_splits(splits, n)
            sets[name] = runs_from_cuts(cuts)
            sets[name + " mirrored"] = runs_from_cuts({total - c for c in cuts})
    return sets


# ---------------------------------------------------------------------------------------------
# Synthetic inputs.
class Problem(object):
    """PATHS paths of `levels_per_path` levels on `columns` points: nu [columns] ascending from 0,
    beta [levels, columns], thickness and temperature [levels], boundaries and surfaces [PATHS]."""
    def __init__(self, columns, levels_per_path, seed, signed=False):
        rng = np.random.default_rng(seed)
        levels = PATHS*levels_per_path
        self.columns, self.levels_per_path, self.levels = columns, levels_per_path, levels
        steps = rng.uniform(0.2, 1.8, size=columns - 1)*(3000./max(columns - 1, 1))
        self.nu = np.concatenate([[0.], np.cumsum(steps)])
        beta = 10.**rng.uniform(-12., 1., size=(levels, columns))
        beta[rng.random(beta.shape) < 0.05] = 0.
        if signed:
            beta[rng.random(beta.shape) < 0.3] *= -1.
        self.beta = beta
        self.thickness = rng.uniform(0.5, 1.5, size=levels)
        self.thickness[1 % levels] = 0.
        self.temperature = rng.uniform(150., 320., size=levels)
        self.boundary_t = np.array([0., 288., 215.])       # path 0: no boundary
        self.boundary_e = np.array([1., 0.9, 0.])
        self.surface_t = np.array([270., 288., 305.])
        self.surface_e = np.array([1., 0.7, 0.])

    def lengths(self, angles):
        """(s_l/mu_k [levels, K] in float64 as the host forms them, weights [K])."""
        mu, weight = flux_angles(angles)
        return self.thickness[:, None]/mu, weight


def value_problem():
    """The extreme-value table: 9 levels per path on 67 columns.  Column j has the beta of group
    j % 4: 0 all zeros; 1 random with s*beta >= 800 in each path's first and last level; 2 random of
    mixed sign; 3 random.  nu[0] = 0; the others leave out where C2 nu/T for T = 1 K and T = 5 K lies
    in (700, 760), where Planck's expm1 overflows in float64 long before the quotient underflows.
    Levels 4 and 5 of every path are at 1 K and 320 K; path 2 enters behind a 5 K boundary, path 1
    behind a 1 K one, and the surfaces follow suit."""
    problem = Problem(67, 9, seed=77)
    rng = np.random.default_rng(78)
    low = np.sort(np.concatenate([rng.uniform(1., 480., 24), rng.uniform(540., 1900., 16)]))
    high = np.sort(np.concatenate([rng.uniform(2000., 2400., 13), rng.uniform(2700., 3000., 13)]))
    problem.nu = np.concatenate([[0.], low, high])
    assert problem.nu.size == 67 and np.all(np.diff(problem.nu) > 0.)
    group = np.arange(67) % 4
    beta = problem.beta
    beta[:, group == 0] = 0.
    problem.thickness[:] = rng.uniform(0.5, 1.5, size=problem.levels)
    problem.thickness[12] = 0.
    for p in range(PATHS):
        for level in (9*p, 9*p + 8):
            beta[level, group == 1] = rng.uniform(800., 5000., size=np.sum(group == 1)) / \
                problem.thickness[level]
        problem.temperature[9*p + 4] = 1.
        problem.temperature[9*p + 5] = 320.
    negative = rng.random(beta.shape) < 0.4
    beta[:, group == 2] = np.where(negative, -beta, beta)[:, group == 2]
    problem.group = group
    problem.boundary_t = np.array([0., 1., 5.])
    problem.boundary_e = np.array([1., 1., 1.])
    problem.surface_t = np.array([288., 1., 5.])
    problem.surface_e = np.array([1., 0.7, 0.])
    return problem


# ---------------------------------------------------------------------------------------------
# The recurrences of include/lbl_amd.h in the float type `kind`, every product and sum rounded as
# written, for all paths at once.  Each returns per flat level the value and its magnitude (the
# same recurrence over absolute values of the terms).
def _sweep_order(levels_per_path, from_last):
    return range(levels_per_path - 1, -1, -1) if from_last else range(levels_per_path)


def _flat(levels_per_path, step):
    return np.arange(PATHS)*levels_per_path + step


def sweep_tau(kind, beta, lengths, levels_per_path, from_last=False):
    """tau = tau + s*beta from 0: (tau, sum |s*beta|) after every level, [levels, columns]."""
    beta, lengths = beta.astype(kind), lengths.astype(kind)
    tau = np.zeros((PATHS, beta.shape[1]), dtype=kind)
    mag = tau.copy()
    out, mags = np.zeros(beta.shape, dtype=kind), np.zeros(beta.shape, dtype=kind)
    for step in _sweep_order(levels_per_path, from_last):
        rows = _flat(levels_per_path, step)
        term = lengths[rows, None]*beta[rows]
        tau = tau + term
        mag = mag + np.abs(term)
        out[rows], mags[rows] = tau, mag
    return out, mags


def planck(kind, nu, temperature):
    nu, temperature = np.asarray(nu, dtype=kind), np.asarray(temperature, dtype=kind)
    c1, c2 = kind(PLANCK_C1), kind(PLANCK_C2)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore", under="ignore"):
        b = (((c1*nu)*nu)*nu)/np.expm1((c2*nu)/temperature)
    return np.where(nu > 0., b, kind(0.))


def brightness(kind, nu, radiance):
    nu, radiance = np.asarray(nu, dtype=kind), np.asarray(radiance, dtype=kind)
    c1, c2 = kind(PLANCK_C1), kind(PLANCK_C2)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore", under="ignore"):
        t = (c2*nu)/np.log1p((((c1*nu)*nu)*nu)/radiance)
    return np.where((nu > 0.) & (radiance > 0.), t, kind(0.))


def flushed(values):
    """Values below float64's range as float64 holds them: 0 (long double reaches 1e-4932, so a
    radiance that has underflowed in every float64 evaluation is still a number there)."""
    values = np.asarray(values)
    return np.where(np.abs(values) < LD("2.4e-324"), values.dtype.type(0.), values)


def brightness_magnitude(kind, nu, radiance, magnitude):
    """The scale of brightness temperature's error: d ln T_b / d ln I <= 1, so an error of
    bound*magnitude in I is at most bound*T_b*magnitude/|I| in T_b."""
    t = brightness(kind, nu, radiance)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0., t*(magnitude/np.abs(radiance)), kind(0.))


def boundary_start(kind, nu, temperature, emissivity):
    """eps*B(nu, T_boundary) per path, 0 where T_boundary is 0: [PATHS, columns]."""
    t = np.asarray(temperature, dtype=kind)[:, None]
    e = np.asarray(emissivity, dtype=kind)[:, None]
    safe = np.where(t > 0., t, kind(1.))
    return np.where(t > 0., e*planck(kind, nu, safe), kind(0.))


def sweep_radiance(kind, nu, beta, lengths, temperature, levels_per_path, from_last=False,
                   start=None):
    """I = I*exp(-x) + B*(-expm1(-x)), x = s*beta, from `start` [PATHS, columns] (None: 0): (I,
    magnitude) after every level, [levels, columns]."""
    beta, lengths = beta.astype(kind), lengths.astype(kind)
    shape = (PATHS, beta.shape[1])
    rad = np.zeros(shape, dtype=kind) if start is None else np.array(start, dtype=kind)
    mag = np.abs(rad)
    out, mags = np.zeros(beta.shape, dtype=kind), np.zeros(beta.shape, dtype=kind)
    for step in _sweep_order(levels_per_path, from_last):
        rows = _flat(levels_per_path, step)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            x = lengths[rows, None]*beta[rows]
            source = planck(kind, nu, temperature[rows, None])*(-np.expm1(-x))
            rad = rad*np.exp(-x) + source
            mag = mag*np.exp(-x) + np.abs(source)
        out[rows], mags[rows] = rad, mag
    return out, mags


def flux_sum(weight, rad):
    """sum_k w_k*I_k from k = 0; rad [..., K, columns]."""
    total = weight[0]*rad[..., 0, :]
    for k in range(1, weight.size):
        total = total + weight[k]*rad[..., k, :]
    return total


FluxSweep = namedtuple("FluxSweep", "flux flux_mag rad rad_mag total total_mag")


def sweep_flux(kind, nu, beta, lengths, weight, temperature, levels_per_path, from_last=False,
               start=None, start_mag=None):
    """K radiances per column from `start` [PATHS, columns] (None: 0, the down sweep): after every
    level F = pi*(sum_k w_k*I_k) [levels, columns] and the radiances [levels, K, columns], with
    magnitudes; total [PATHS, columns] = sum_k w_k*I_k of each path's last level in sweep order."""
    beta, lengths = beta.astype(kind), lengths.astype(kind)
    weight = weight.astype(kind)
    angles = weight.size
    shape = (PATHS, angles, beta.shape[1])
    rad = np.zeros(shape, dtype=kind)
    mag = np.zeros(shape, dtype=kind)
    if start is not None:
        rad = rad + np.asarray(start, dtype=kind)[:, None, :]
        mag = mag + np.asarray(np.abs(start) if start_mag is None else start_mag,
                               dtype=kind)[:, None, :]
    levels = beta.shape[0]
    flux, flux_mag = (np.zeros(beta.shape, dtype=kind) for _ in range(2))
    rads, rad_mags = (np.zeros((levels,) + shape[1:], dtype=kind) for _ in range(2))
    pi = kind(FLUX_PI)
    for step in _sweep_order(levels_per_path, from_last):
        rows = _flat(levels_per_path, step)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            x = lengths[rows][:, :, None]*beta[rows][:, None, :]
            source = planck(kind, nu, temperature[rows, None])[:, None, :]*(-np.expm1(-x))
            rad = rad*np.exp(-x) + source
            mag = mag*np.exp(-x) + np.abs(source)
        rads[rows], rad_mags[rows] = rad, mag
        flux[rows], flux_mag[rows] = pi*flux_sum(weight, rad), pi*flux_sum(weight, mag)
    return FluxSweep(flux, flux_mag, rads, rad_mags, flux_sum(weight, rad), flux_sum(weight, mag))


def surface_start(kind, nu, temperature, emissivity, reflection, reflection_mag):
    """eps*B(nu, T_s) + (1 - eps)*R and its magnitude: [PATHS, columns]."""
    e = np.asarray(emissivity, dtype=kind)[:, None]
    emitted = e*planck(kind, nu, np.asarray(temperature, dtype=kind)[:, None])
    one = kind(1.)
    return emitted + (one - e)*reflection, np.abs(emitted) + (one - e)*reflection_mag


def band_means(kind, values, band_start):
    """Arithmetic means of [rows, columns] over the bands in `kind`: NaN for an empty band."""
    values = np.asarray(values, dtype=kind)
    out = np.full((values.shape[0], len(band_start) - 1), np.nan, dtype=kind)
    for b in range(len(band_start) - 1):
        if band_start[b + 1] > band_start[b]:
            out[:, b] = np.sum(values[:, band_start[b]:band_start[b + 1]], axis=1) / \
                kind(band_start[b + 1] - band_start[b])
    return out


def pattern(values):
    """Where values (seen as float64) are NaN, +inf, -inf and exactly zero."""
    with np.errstate(over="ignore", under="ignore"):
        v = np.asarray(values).astype(np.float64)
    return np.isnan(v), v == np.inf, v == -np.inf, v == 0.


def same_pattern(a, b):
    return all(np.array_equal(x, y) for x, y in zip(pattern(a), pattern(b)))


# ---------------------------------------------------------------------------------------------
# The case tables.
COLUMNS = (1, 2, 3, 511, 512, 513, 1031, 8193)      # a block is 512 columns
LAYOUT_COLUMNS = (1, 3, 512, 513, 1031)             # every layout on these
LEVELS = (1, 7, 8, 9, 19)                           # kPathAhead = 8 rows in flight
LEVELS_MANY = (3, 4, 5, 11)                         # K > 4: 4 rows in flight
RUN_COLUMNS = 1031
ANGLES = tuple(range(1, FLUX_MAX_ANGLES + 1))
ANGLE_COLUMNS = 131


def angle_levels(angles):
    """A depth with two full batches and a remainder for path_flux_kernel<., angles>."""
    return 2*flux_ahead(angles) + 3


def run_cases(kernel):
    """[(levels_per_path, angles or None, {name: runs})] of the levels-and-runs table."""
    if kernel != "flux":
        return [(n, None, run_sets(n, PATH_AHEAD if n == 19 else None)) for n in LEVELS]
    few = [(n, 3, run_sets(n, PATH_AHEAD if n == 19 else None)) for n in LEVELS]
    many = [(n, 6, run_sets(n, FLUX_AHEAD_MANY if n == 11 else None)) for n in LEVELS_MANY]
    return few + many


def kernel_ahead(kernel, angles):
    return flux_ahead(angles) if kernel == "flux" else PATH_AHEAD


# Band sets: {columns: band_start}.  On 8193 columns: an empty band at column 0, bands of 1, 63, 64
# and 65 columns, one that ends exactly on 4096, one that starts on it and is a whole segment,
# an empty band in the middle, one that spans three segments (4000 .. 8193 is cut at 4096 and
# 8192), and an empty band at `columns`.  On 67 columns (odd): the last band ends at `columns`.
BANDS = {
    8193: np.array([0, 0, 1, 64, 128, 193, 4096, 8192, 8192, 8193, 8193], dtype=np.int64),
    67: np.array([0, 0, 5, 5, 6, 66, 67], dtype=np.int64),
}
BANDS_SPANNING = np.array([0, 4000, 8193, 8193], dtype=np.int64)      # three segments in one band
BAND_SETS = (("8193", 8193, BANDS[8193]), ("8193 spanning", 8193, BANDS_SPANNING),
             ("67", 67, BANDS[67]))
