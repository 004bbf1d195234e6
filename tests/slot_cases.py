"""What tests/test_slot_cases_host.py (CPU) and tests/test_gpu_slot_shapes.py (GPU) share: builders
of cross-section bands and spectral grids aimed at the sizes the kernels of csrc/xsec.h and
csrc/continuum.h branch on, and numpy restatements ("mirrors") of the route decisions those kernels
take -- per workgroup of xsec_interp_kernel the search window and whether it is staged in LDS, per
wavefront run of continuum_interp_kernel / group_interp_kernel the class of the run and the route
add_band takes.  The mirrors only prove that a case reaches the branch it is named for; expected
values come from oracle/xsec_oracle.py and oracle/mt_ckd_oracle.py alone."""
from collections import namedtuple

import numpy as np

SPEED_OF_LIGHT = 299792458.0    # kSpeedOfLight; Hz = cm-1 * SPEED_OF_LIGHT * 100, in that order
XSEC_STAGE = 1024               # kXsecStage
XSEC_MAX_BANDS = 16             # kMaxXsecBands
MODEL_THREADS = 1024            # kModelThreads

# The two instantiations lbl_xsec_compute and lbl_continuum_compute launch: <4, 1> for one level,
# <2, 4> for more (5 levels: one full group of four and a partial one).  `points`: grid points of a
# workgroup of xsec_interp_kernel; `run`: of a wavefront of continuum_interp_kernel (64 PT).
Instance = namedtuple("Instance", "name pt levels points run")
INSTANCES = {x.name: x for x in (Instance("4x1", 4, 1, 1024, 256), Instance("2x4", 2, 5, 512, 128))}

SIZES = (2, 3, 63, 64, 65, 128, 129, 1023, 1024, 1025, 4096, 4097)
COUNTS = (1, 2, 3, 15, 16)
TAILS = (1, 2, 3, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
WINDOWS = (1023, 1024, 1025, 3000)
LEVEL_COUNTS = (2, 3, 4, 8, 9)      # run on one case beside 1 and 5
MODEL_SIZES = (2, 1023, 1024, 1025, 4097)


def hz(wavenumber):
    """The frequency the kernel and the reference form for a wavenumber (cross_section.py:32)."""
    return np.asarray(wavenumber, dtype=np.float64)*SPEED_OF_LIGHT*100


def levels(count, period=None):
    """(temperature [K], pressure [Pa]) of `count` levels, repeating with `period` if given."""
    i = np.arange(count) % (period or count)
    return 296. - 11.*i, 1.e5*np.exp(-0.6*i)


# ---------------------------------------------------------------------------------------------
# Cross-section bands.
def xsec_band(size, lower, seed, kind="noisy", spacing=0.05):
    """(frequency [Hz], coefficients [4, size]) on unevenly spaced frequencies from `lower` [cm-1]
    up, the recipe of synthetic.cross_section_bands: a two-peak shape of 1e-22 m2 with noise of
    2e-24 that drives the wings negative ("noisy": clip and rescale).  "negative_sum": the fit sums
    negative with its peak still positive (clip without rescale); "no_negative": lifted clear of
    zero (no clipping at all)."""
    rng = np.random.default_rng(5000 + seed)
    steps = rng.uniform(0.5, 1.5, size)
    wavenumber = lower + spacing*(np.cumsum(steps) - steps[0])
    f = (np.arange(size) + 0.5)/size
    shape = 1e-22*(np.exp(-((f - 0.4)/0.1)**2) + 0.5*np.exp(-((f - 0.7)/0.05)**2))
    coefficients = np.zeros((4, size))
    coefficients[0] = shape + 2e-24*rng.standard_normal(size)
    coefficients[1] = 1e-26*rng.standard_normal(size)
    coefficients[2] = 1e-29*rng.standard_normal(size)
    coefficients[3] = 1e-29*rng.standard_normal(size)
    if kind == "negative_sum":
        coefficients[0] -= 6e-23
    elif kind == "no_negative":
        coefficients[0] += 6e-23
        coefficients[1:] *= 0.1
    return hz(wavenumber), coefficients


def band_wavenumbers(band):
    return band[0]/(SPEED_OF_LIGHT*100)


def molecule(size, count, seed=0):
    """`count` bands, the first of `size` frequencies, the others taking the following entries of
    SIZES in turn (bands 3 and 4 at least 129).  Band 1 starts in the middle of band 0 (overlap),
    band 2 starts on the very frequency band 1 ends on (a shared end), the others lie apart; band 3
    sums negative and band 4 has no negative value."""
    first = SIZES.index(size)
    bands, upper = [], 600.
    for k in range(count):
        n = SIZES[(first + k) % len(SIZES)]
        kind = {3: "negative_sum", 4: "no_negative"}.get(k, "noisy")
        if kind != "noisy":
            n = max(n, 129)                 # (a peak and wings need some frequencies)
        if k == 1:
            w = band_wavenumbers(bands[0])
            lower = 0.5*(w[0] + w[-1])
        elif k == 2:
            lower = 0.                      # moved onto band 1's last frequency below
        else:
            lower = upper + 5.
        frequency, coefficients = xsec_band(n, lower, 100*seed + 16*first + k, kind)
        if k == 2:
            frequency = frequency - frequency[0] + bands[1][0][-1]
            assert frequency[0] == bands[1][0][-1]
        bands.append((frequency, coefficients))
        upper = max(upper, frequency[-1]/(SPEED_OF_LIGHT*100))
    return bands


def model_bands():
    """The bands engine.xsec_bands is checked on: MODEL_SIZES noisy, one that sums negative, one
    without a negative value."""
    bands = [xsec_band(n, 600. + 300.*i, 900 + i) for i, n in enumerate(MODEL_SIZES)]
    bands.append(xsec_band(1025, 2400., 950, "negative_sum"))
    bands.append(xsec_band(1023, 2700., 951, "no_negative"))
    return bands


def exact_knots(frequency):
    """Wavenumbers [cm-1] that convert back onto the band's frequencies bit for bit, and which of
    the frequencies have one (among the quotient and its four nearest neighbours)."""
    guess = frequency/(SPEED_OF_LIGHT*100)
    found = np.zeros(frequency.size, dtype=bool)
    out = guess.copy()
    candidates = [guess]
    for direction in (-np.inf, np.inf):
        step = np.nextafter(guess, direction)
        candidates += [step, np.nextafter(step, direction)]
    for candidate in candidates:
        hit = (hz(candidate) == frequency) & ~found
        out[hit] = candidate[hit]
        found |= hit
    return out, found


def all_knots(bands):
    """Every frequency of every band that has an exact wavenumber, as wavenumbers, ascending."""
    pieces = []
    for frequency, _ in bands:
        w, ok = exact_knots(frequency)
        pieces.append(w[ok])
    return np.unique(np.concatenate(pieces))


def span(bands):
    return (min(band_wavenumbers(b)[0] for b in bands), max(band_wavenumbers(b)[-1] for b in bands))


# ---------------------------------------------------------------------------------------------
# Grids for cross-sections.
def knots_grid(bands, at_least=2600):
    """Every knot of every band with its nextafter neighbours on both sides, ascending; filled up
    with evenly spaced points from below the first band to above the last where the knots are few,
    so that both instantiations get more than two workgroups."""
    knots = all_knots(bands)
    points = [knots, np.nextafter(knots, -np.inf), np.nextafter(knots, np.inf)]
    lower, upper = span(bands)
    missing = at_least - 3*knots.size
    if missing > 0:
        points.append(np.linspace(lower - 1., upper + 1., missing))
    return np.unique(np.concatenate(points))


EDGE_VARIANTS = ("below|on", "on|above", "on|next", "2below|below", "above|2above")


def edges_grid(bands, groups=12):
    """An ascending grid whose points 512 m - 1 and 512 m (m = 1 ...: the last point of a workgroup
    and the first of the next, for <2,4>; every second of them for <4,1>) are a knot and its
    neighbours by EDGE_VARIANTS in turn: "below|on" = one ulp below the knot, then the knot.
    Returns (grid, [(m, variant, knot)])."""
    knots = all_knots(bands)
    groups = min(groups, knots.size)
    chosen = np.unique(np.round(np.linspace(0, knots.size - 1, groups)).astype(int))
    below, above = np.nextafter(knots, -np.inf), np.nextafter(knots, np.inf)
    pieces, plan = [], []
    previous = knots[0] - 2.
    for m, a in enumerate(chosen, start=1):
        variant = EDGE_VARIANTS[(m - 1) % len(EDGE_VARIANTS)]
        if variant == "on|next" and (a + 1 >= knots.size or (m < chosen.size and chosen[m] <= a + 1)):
            variant = "below|on"
        pair = {"below|on": (below[a], knots[a]), "on|above": (knots[a], above[a]),
                "on|next": (knots[a], knots[min(a + 1, knots.size - 1)]),
                "2below|below": (np.nextafter(below[a], -np.inf), below[a]),
                "above|2above": (above[a], np.nextafter(above[a], np.inf))}[variant]
        fill = 511 if m == 1 else 510
        assert previous < pair[0]
        pieces.append(np.linspace(previous, pair[0], fill + 2)[1:-1])
        pieces.append(np.asarray(pair))
        plan.append((m, variant, knots[a]))
        previous = pair[1]
    pieces.append(np.linspace(previous, previous + 2., 302)[1:])
    grid = np.concatenate(pieces)
    assert np.all(grid[:-1] < grid[1:])
    return grid, plan


def window_band():
    """The band the window-size grids are cut from: 4097 frequencies."""
    return xsec_band(4097, 700., 977)


def window_grid(band, length, instance, from_start=False):
    """An ascending grid whose FIRST workgroup of `instance` stages exactly `length` frequencies:
    its first point one ulp above knot a (w0 = a + 1, the extra element is the knot itself), its
    last one ulp above knot a + length - 1 (w1 = a + length).  from_start: the first point lies
    below the band (w0 = 0, nothing in front to stage) and the last above knot length - 1.  A
    second, partial workgroup follows."""
    w, ok = exact_knots(band[0])
    assert ok.all()
    a = 40
    def just_above(k):
        x = np.nextafter(w[k], np.inf)
        while not hz(x) > band[0][k]:
            x = np.nextafter(x, np.inf)
        return x

    first = w[0] - 0.5 if from_start else just_above(a)
    last = just_above(length - 1 if from_start else a + length - 1)
    head = np.linspace(first, last, instance.points)
    head[0], head[-1] = first, last
    return np.concatenate([head, np.linspace(last, last + 1., 101)[1:]])


def tail_grid(bands, n, seed=0):
    """`n` unevenly spaced ascending points from below the bands to above them."""
    lower, upper = span(bands)
    rng = np.random.default_rng(6000 + seed + n)
    return np.sort(rng.uniform(lower - 0.5, upper + 0.5, n))


def order_grids(bands):
    """The same kind of points in other orders and positions; "shuffled" is
    ascending[permutation]."""
    ascending = knots_grid(bands)
    lower, upper = span(bands)
    permutation = np.random.default_rng(77).permutation(ascending.size)
    grids = {
        "ascending": ascending,
        "descending": ascending[::-1].copy(),
        "shuffled": ascending[permutation],
        "repeated neighbours": np.repeat(ascending, 2)[:-1],
        "zero and negative": np.concatenate([[-lower, -1e-3, -0., 0.], ascending]),
        "below every band": np.linspace(1., np.nextafter(lower, -np.inf), 1500),
        "above every band": np.linspace(np.nextafter(upper, np.inf), upper + 100., 1500),
    }
    return grids, permutation


def outside_every_band(bands, grid):
    """Points where the reference adds nothing: the frequency lies in no band."""
    x = hz(grid)
    inside = np.zeros(x.size, dtype=bool)
    for frequency, _ in bands:
        inside |= (x >= frequency[0]) & (x <= frequency[-1])
    return ~inside


# ---------------------------------------------------------------------------------------------
# Mirror of xsec_interp_kernel's head: the window of every (workgroup, band).
Window = namedtuple("Window", "group band touches w0 w1 base length in_lds")


def is_ascending(grid):
    return bool(np.all(grid[:-1] <= grid[1:]))      # std::is_sorted (lbl_grid_load)


def xsec_windows(bands, grid, instance):
    x = hz(grid)
    ascending = is_ascending(grid)
    out = []
    for group in range(-(-grid.size//instance.points)):
        first = group*instance.points
        last = min(first + instance.points, grid.size) - 1
        for k, (f, _) in enumerate(bands):
            if ascending:
                touches = bool(x[last] >= f[0] and x[first] <= f[-1])
                w0 = int(np.searchsorted(f, x[first], side="left")) if touches else -1
                w1 = int(np.searchsorted(f, x[last], side="left")) if touches else -1
            else:
                touches, w0, w1 = True, 0, f.size
            base = max(w0 - 1, 0)
            length = w1 - base
            out.append(Window(group, k, touches, w0, w1, base, length,
                              touches and length <= XSEC_STAGE))
    return out


def boundary_points(grid, instance):
    """(index of the first point, index of the last point) of every workgroup."""
    return [(g*instance.points, min((g + 1)*instance.points, grid.size) - 1)
            for g in range(-(-grid.size//instance.points))]


# ---------------------------------------------------------------------------------------------
# Continua: arithmetic grids against one band's coarse grid, and the class of every wavefront run.
OWNERS = ("H2OForeign", "H2OSelf", "CO2", "N2", "O2", "O3")
GROUPS = (("H2OForeign", "H2OSelf"), OWNERS)
# The band of each continuum the grids are aimed at: its first, whose lower bound and resolution
# are whole numbers, so that start + i*step below is exact and lands on lower + j*resolution bit
# for bit.  Its knot at 0 cm-1 (H2O, CO2, N2: the radiation term vanishes) or its last knot (O2, O3:
# the table ends in 0) holds an exact 0 beside a non-zero neighbour.
TARGET_BAND = 0
RUN_CLASSES = ("one interval", "knot inside", "first is a knot", "last is a knot",
               "straddles the first knot", "straddles the last knot", "ends on the last knot",
               "outside", "partial")

Coarse = namedtuple("Coarse", "lower resolution size")
Run = namedtuple("Run", "index classes route")


def coarse_of(knots):
    """Coarse(lower, resolution, size) of a band from its knots (oracle Continuum.bands[k][0])."""
    return Coarse(float(knots[0]), float(knots[1] - knots[0]), int(knots.size))


def run_grids(coarse, instance):
    """{name: numpy.arange grid} for one band and one instantiation.  R = instance.run points make
    a wavefront's run; the step is resolution / R (or / 2R), so a run is as long as a coarse
    interval (or half of one) and where it starts decides what it holds."""
    lower, res, size = coarse
    last = lower + (size - 1)*res
    R = instance.run
    step, half = res/R, res/(2*R)

    def arange(start, runs, step):
        n = int(runs*R) + R//2 + 3          # (a partial last run)
        return start + np.arange(n)*step

    grids = {
        # runs 0, 1 below the band; from run 2 on every run starts on a knot and ends one step
        # below the next
        "low aligned": arange(lower - 2*res, 6, step),
        # every run ends on a knot: run 1 on the first (it straddles the band's edge), run 3 on the
        # knot at lower + 2 resolution
        "low ending on knots": arange(lower - 2*res + step, 6, step),
        # every run holds a knot in its middle; run 1 the first knot
        "low knots inside": arange(lower - 2*res + (R//2)*step, 6, step),
        # half an interval per run, 3 steps off the knots: no run touches a knot
        "low between knots": arange(lower - res + 3*half, 8, half),
        # run 2 ends exactly on the last knot, run 3 lies above the band
        "high ending on knots": arange(last - 3*res + step, 5, step),
        # run 2 holds the last knot in its middle
        "high knots inside": arange(last - 3*res + (R//2)*step, 5, step),
        "high aligned": arange(last - 3*res, 5, step),
    }
    ascending = grids["low ending on knots"]
    grids["descending"] = ascending[-1] + np.arange(ascending.size)*(-step)
    grids["linspace"] = np.linspace(ascending[0], ascending[-1], ascending.size + 1)
    grids["short"] = (lower + res + step) + np.arange(50)*step
    return grids


def arithmetic(grid):
    """(arithmetic, start, step) as lbl_grid_load decides it."""
    if grid.size < 2:
        return False, 0., 0.
    start, step = grid[0], grid[1] - grid[0]
    offsets = np.arange(grid.size).astype(np.float64)*step
    return bool(np.all(start + offsets == grid)), float(start), float(step)


def continuum_runs(coarse, grid, instance):
    """Per wavefront run of `instance`: the RUN_CLASSES it belongs to against the band `coarse`
    and the route of add_band ("skip", "fast", "points")."""
    lower, res, size = coarse
    knots = lower + np.arange(size).astype(np.float64)*res      # lower + j*resolution
    x_last = knots[-1]
    is_arithmetic, start, step = arithmetic(grid)
    R = instance.run
    out = []
    for r in range(-(-grid.size//R)):
        first, last = r*R, r*R + R - 1
        partial = last >= grid.size
        end = min(last, grid.size - 1)
        # (wavenumber_at: the product rounded, then the sum)
        lo = start + np.float64(first)*step if is_arithmetic else grid[first]
        hi = start + np.float64(end)*step if is_arithmetic else grid[end]
        assert lo == grid[first] and hi == grid[end]
        low, high = min(lo, hi), max(lo, hi)
        classes = set()
        if partial:
            classes.add("partial")
        if high < lower or low > x_last:
            classes.add("outside")
        else:
            if low < lower <= high:
                classes.add("straddles the first knot")
            if low <= x_last < high:
                classes.add("straddles the last knot")
            if low >= lower and high <= x_last:
                if high == x_last:
                    classes.add("ends on the last knot")
                if np.any(knots == lo):
                    classes.add("first is a knot")
                if np.any(knots == hi):
                    classes.add("last is a knot")
                if np.any((knots > low) & (knots < high)):
                    classes.add("knot inside")
                j_lo = int(np.searchsorted(knots, low, side="right")) - 1
                if j_lo < size - 1 and high < knots[j_lo + 1]:
                    classes.add("one interval")
        usable = is_arithmetic and step > 0. and not partial
        if not usable:
            route = "points"
        elif "outside" in classes:
            route = "skip"
        else:
            route = "fast" if "one interval" in classes else "points"
        out.append(Run(r, frozenset(classes), route))
    return out


def zero_knots(knots, spectrum):
    """Knots whose coarse value is exactly 0 beside a predecessor that is not."""
    at = np.flatnonzero((spectrum[1:] == 0.) & (spectrum[:-1] != 0.)) + 1
    return knots[at]
