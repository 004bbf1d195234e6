"""Inputs for the line-by-line tests of the far-field series (csrc/farfield.h), and a numpy mirror
of what decides which (line, tile) pairs it takes and of its arithmetic.

The partition mirror restates, from the inputs of a call alone, pick_tiling (lanes_plans.inc),
tile_bounds and tile_centre (accumulate.h), the eight search keys and the clamps of schedule_tile
(tile_schedule.h) and the group cuts and the four tile pieces of farfield_series_kernel
(farfield.h).  For every (line, tile) of a level it names one class:

    direct          [f1, f2): evaluated point by point (fast ranges and core range)
    clipped         [lo, a1) and [a2, hi): the window may end inside the tile
    tile near       [l2, f1) and [f2, r1): the tile's own series, nearer than the group's limit
    tile cover      [a1, l1) and [r2, a2): the tile's own series, covers this tile but not the group
    group           [a1, g1) and [g2, a2) of the group: expanded about the group's centre
    outside         no overlap

The series mirror restates the arithmetic -- the recurrence of series_terms, the sums over the 64
lanes (wave_ops.h: wave_sums pairs lane l with l ^ 1, ^ 2, ..., a balanced tree) and over the four
wavefronts, the Taylor shift from the group's centre to the tile's and the Horner evaluation of
accumulate.h -- once in float64 and once in long double.  It measures the rounding allowance E_CPU
of the GPU tests; the reference of those tests is the exact Lorentz term, or the CPU oracle.

truncation(rho) = rho^21 (22 + 21 rho) is the relative remainder of the 21-term series of
1/(a - u)^2 at u = -rho a (the side of the tile away from the line) for gamma << a:
sum_{k >= 21} (k + 1)(-rho)^k (1 + rho)^2.  6.2e-12 at the hand-over ratio rho = 1/4.
"""
from types import SimpleNamespace

import numpy as np

FAR_RATIO = 4.          # accumulate.h: LBL_FAR_RATIO
FAR_TERMS = 21          # accumulate.h: LBL_FAR_TERMS
FAR_GROUP = 4           # farfield.h: kFarGroup
INLINE_LEVELS = 4       # tile_schedule.h: kInlineLevels
ROUNDING = 1.e-12       # the direct kernel against the oracle (tests/test_gpu_core_quotient.py)
STEP = 1.e-4            # how far past (or inside) a cut a hand-over line is placed [cm-1]

# The worst |float64 mirror - long-double mirror|/value over every series tile of the one-line
# cases (tests/test_farfield_cases_host.py measures and prints it, and holds this record to it).
E_CPU = 1.1e-15

DIRECT, CLIPPED, TILE_NEAR, TILE_COVER, GROUP, OUTSIDE = range(6)
CLASS_NAMES = ("direct", "clipped", "tile near", "tile cover", "group", "outside")
SERIES_CLASSES = (TILE_NEAR, TILE_COVER, GROUP)
MUTATIONS = ("g1 by one line", "l1 and l2 swapped", "shift_max ignored")

X = 4.e-4
ONE_LINE_LEVELS = ((296., 101325.), (296., 10.))
FIVE_LEVELS = ((220., 10.), (240., 1000.), (260., 1.e4), (280., 5.e4), (300., 101325.))


def truncation(rho):
    return rho**FAR_TERMS*(FAR_TERMS + 1 + FAR_TERMS*rho)


TABLE_TOLERANCE = truncation(0.25) + ROUNDING


# ---------------------------------------------------------------------------------------------
# Cases.  The names carry the tile and group counts the tiling mirror must find.
def _case(name, span, points, v0=1000, npv=1000, cut_off=25, **expect):
    return SimpleNamespace(name=name, v0=v0, vn=v0 + span, npv=npv, cut_off=cut_off,
                           points=points, n=span*npv, expect=expect)


CASES = {
    "A": _case("A: 38 aligned tiles of 500, 10 groups, last of 2", 19, 8,
               aligned=1, length=500, n_tiles=38, n_groups=10, p=8),
    "B": _case("B: 6 aligned tiles, 2 groups", 3, 8,
               aligned=1, length=500, n_tiles=6, n_groups=2, p=8),
    "C": _case("C: 80 aligned tiles of 63 and 55, 20 groups", 5, 1,
               aligned=1, length=63, n_tiles=80, n_groups=20, p=1),
    "D": _case("D: 10 unaligned tiles of 512, last 292, 3 groups", 7, 8, npv=700,
               aligned=0, length=512, n_tiles=10, n_groups=3, p=8),
    "E": _case("E: 32 unaligned tiles of 128, 8 groups", 40, 0, npv=100,
               aligned=0, length=128, n_tiles=32, n_groups=8, p=2),
    "E1000": _case("E1000: default tiling at 1000 points, 24 aligned tiles, 6 groups", 12, 0,
                   aligned=1, length=500, n_tiles=24, n_groups=6, p=8),
    "H": _case("H: 24 aligned tiles of 125 at 8000 cm-1, 6 groups", 3, 2, v0=8000,
               aligned=1, length=125, n_tiles=24, n_groups=6, p=2),
}
ONE_LINE_CASES = ("A", "C", "D", "H")
TABLE_CASES = ("A", "B", "C", "D", "E", "E1000", "H")
CUT_OFFS = (1, 2, 3, 4, 5, 6)


def with_cut_off(case, cut_off):
    out = SimpleNamespace(**vars(case))
    out.cut_off = cut_off
    out.name = "%s, cut_off %d" % (case.name, cut_off)
    return out


# ---------------------------------------------------------------------------------------------
# Tiling (lanes_plans.inc: pick_tiling; compute_stages.inc: shape_of; accumulate.h).
def pick_tiling(forced, farfield, npv, n):
    is_forced = forced in (1, 2, 4, 8)
    for candidate in (8, 4, 2, 1):
        p = forced if is_forced else candidate
        width = 64*p
        per_cell = (npv + width - 1)//width
        waste = float(per_cell)*width/npv - 1.
        if farfield and waste <= 0.06:
            return SimpleNamespace(p=p, aligned=1, per_cell=per_cell,
                                   length=(npv + per_cell - 1)//per_cell,
                                   n_tiles=(n//npv)*per_cell)
        if is_forced:
            break
    p = forced
    if not is_forced:
        p = 8 if (npv >= 400 and farfield) else 2 if (npv >= 100 and farfield) else \
            4 if npv >= 100 else 2 if npv >= 10 else 1
    return SimpleNamespace(p=p, aligned=0, per_cell=0, length=64*p,
                           n_tiles=(n + 64*p - 1)//(64*p))


def call_tiling(case):
    """(tiling, farfield) of a call with the series asked for: tiles so wide that no line of a
    window is FAR_RATIO half-widths away switch it off."""
    tiling = pick_tiling(case.points, 1, case.npv, case.n)
    if FAR_RATIO*0.5*float(tiling.length) >= float(case.cut_off)*case.npv:
        return pick_tiling(case.points, 0, case.npv, case.n), 0
    return tiling, 1


def tile_bounds(tiling, tile, npv, n):
    if tiling.aligned:
        cell = tile//tiling.per_cell
        sub = tile - cell*tiling.per_cell
        i0 = cell*npv + sub*tiling.length
        i1 = min(i0 + tiling.length - 1, (cell + 1)*npv - 1)
    else:
        i0 = tile*tiling.length
        i1 = i0 + tiling.length - 1
    return i0, min(i1, n - 1)


def wavenumber(case, i):
    """absorption.c:39: v0 + i*dv, the product rounded, then the sum."""
    return float(case.v0) + np.asarray(i, dtype=np.float64)*(1./case.npv)


def n_groups_of(tiling):
    return (tiling.n_tiles + FAR_GROUP - 1)//FAR_GROUP


def group_bounds(case, tiling, group):
    t0 = group*FAR_GROUP
    t1 = min(t0 + FAR_GROUP, tiling.n_tiles) - 1
    return tile_bounds(tiling, t0, case.npv, case.n)[0], tile_bounds(tiling, t1, case.npv, case.n)[1]


# ---------------------------------------------------------------------------------------------
# Level scalars (lanes_plans.inc: fill_level).
def level_scalars(table, temperature, pressure):
    p_atm = pressure*9.86923e-6
    mass = table.mass_by_slot()
    slots = sorted({(10 if int(i) == 0 else int(i)) - 1 for i in table.local_iso_id})
    widest = max(np.sqrt(2*np.log(2)*8314.472*temperature/mass[s]) for s in slots)
    biggest = float(np.max(np.abs(table.delta_air))) if table.num_lines else 0.
    return SimpleNamespace(
        temperature=temperature, pressure=pressure, p_atm=p_atm,
        shift_max=abs(p_atm)*biggest*(1. + 1.e-12) + 1.e-12,
        core_reach=123.4/np.sqrt(np.log(2.))/2.99792458e8*widest*(1. + 1.e-9))


def far_radius(lv, v_lo, v_hi, shift=True):
    """(centre, radius, core, half, which side of fmax set the radius): schedule_tile and its
    copy in farfield_series_kernel."""
    smax = lv.shift_max if shift else 0.
    kk = lv.core_reach
    assert kk < 0.5
    core = kk*(v_hi + smax)/(1. - kk)*(1. + 1.e-9) + smax + 1.e-9
    half = 0.5*(v_hi - v_lo)
    side = "core" if core + half > FAR_RATIO*half else "ratio"
    radius = max(FAR_RATIO*half, core + half)*(1. + 1.e-9) + 1.e-6
    return 0.5*(v_lo + v_hi), radius, core, half, side


def _clamp(x, lo, hi):
    return min(max(x, lo), hi)


def schedule_keys(case, tiling, lv, tile, shift=True):
    """(s, keys) of a tile: its bounds, centre and radius, and the eight (key, above) pairs
    schedule_tile searches for, in the order of TileSchedule (lo a1 c1 c2 a2 hi f1 f2).  `above`:
    the first index with nu > key, else with nu >= key."""
    i0, i1 = tile_bounds(tiling, tile, case.npv, case.n)
    smax = lv.shift_max if shift else 0.
    npv, v0, cut = case.npv, case.v0, case.cut_off
    any_lo = float((i0 + npv - 1)//npv + v0 - cut - 1)
    any_hi = float(i1//npv + v0 + cut)
    full_lo = float((i1 + npv - 1)//npv + v0 - cut - 1)
    full_hi = float(i0//npv + v0 + cut)
    v_lo, v_hi = float(wavenumber(case, i0)), float(wavenumber(case, i1))
    u0, radius, core, half, side = far_radius(lv, v_lo, v_hi, shift)
    s = SimpleNamespace(i0=i0, i1=i1, v_lo=v_lo, v_hi=v_hi, u0=u0, radius=radius, side=side,
                        half=half, core=core)
    keys = ((any_lo - smax, False), (full_lo + smax, False), (v_lo - core, False),
            (v_hi + core, True), (full_hi + 1. - smax, False), (any_hi + 1. + smax, False),
            (u0 - radius - smax, True), (u0 + radius + smax, False))
    return s, keys


def clamp_schedule(s, found, farfield):
    """The clamps of schedule_tile on the eight indices found for schedule_keys, into s."""
    s.lo, s.a1, s.c1, s.c2, s.a2, s.hi, f1, f2 = found
    if s.hi < s.lo:
        s.hi = s.lo
    s.a1 = _clamp(s.a1, s.lo, s.hi)
    s.a2 = _clamp(s.a2, s.a1, s.hi)
    s.c1 = _clamp(s.c1, s.a1, s.a2)
    s.c2 = _clamp(s.c2, s.c1, s.a2)
    s.f1, s.f2 = s.a1, s.a2
    if farfield:
        s.f1 = _clamp(f1, s.a1, s.c1)
        s.f2 = _clamp(f2, s.c2, s.a2)
    return s


def schedule_tile(case, tiling, farfield, nu, lv, tile, shift=True):
    """TileSchedule of tile_schedule.h, by the same keys and clamps."""
    s, keys = schedule_keys(case, tiling, lv, tile, shift)
    found = [int(np.searchsorted(nu, key, "right" if above else "left")) for key, above in keys]
    return clamp_schedule(s, found, farfield)


def partition(case, table, temperature, pressure, mutation=None):
    """Everything the series kernels decide for one level of a call on `case`: the tiling, the
    schedule of every tile, the cuts of every group, the pieces of every tile, the class and the
    count of every (tile, line)."""
    assert mutation is None or mutation in MUTATIONS
    nu = np.asarray(table.nu, dtype=np.float64)
    assert np.all(np.diff(nu) >= 0.)
    n_lines = nu.size
    lv = level_scalars(table, temperature, pressure)
    tiling, farfield = call_tiling(case)
    shift = mutation != "shift_max ignored"
    smax = lv.shift_max if shift else 0.
    tiles = [schedule_tile(case, tiling, farfield, nu, lv, t, shift) for t in range(tiling.n_tiles)]
    groups = []
    classes = np.full((tiling.n_tiles, n_lines), OUTSIDE, dtype=np.int8)
    count = np.zeros((tiling.n_tiles, n_lines), dtype=np.int32)

    def mark(tile, first, end, kind):
        if end > first:
            classes[tile, first:end] = kind
            count[tile, first:end] += 1

    for group in range(n_groups_of(tiling) if farfield else 0):
        t0, t1 = group*FAR_GROUP, min(group*FAR_GROUP + FAR_GROUP, tiling.n_tiles)
        i0, i1 = group_bounds(case, tiling, group)
        v_lo, v_hi = float(wavenumber(case, i0)), float(wavenumber(case, i1))
        centre, radius, core, half, side = far_radius(lv, v_lo, v_hi, shift)
        a1 = max(tiles[t].a1 for t in range(t0, t1))
        a2 = min(tiles[t].a2 for t in range(t0, t1))
        f1 = min(tiles[t].f1 for t in range(t0, t1))
        f2 = max(tiles[t].f2 for t in range(t0, t1))
        # wave_search<true>(nu, a1, f1, x) and <false>(nu, f2, a2, x): confined to their range.
        g1 = _clamp(int(np.searchsorted(nu, centre - radius - smax, "right")), a1, f1) \
            if f1 > a1 else a1
        g2 = _clamp(int(np.searchsorted(nu, centre + radius + smax, "left")), f2, a2) \
            if a2 > f2 else a2
        if mutation == "g1 by one line" and g1 < f1:
            g1 += 1         # the nearest line the group must leave to its tiles
        groups.append(SimpleNamespace(t0=t0, t1=t1, i0=i0, i1=i1, v_lo=v_lo, v_hi=v_hi,
                                      centre=centre, radius=radius, side=side, half=half,
                                      a1=a1, g1=g1, g2=g2, a2=a2))
    for t, s in enumerate(tiles):
        mark(t, s.lo, s.a1, CLIPPED)
        mark(t, s.a2, s.hi, CLIPPED)
        mark(t, s.f1, s.f2, DIRECT)
        if not farfield:
            s.pieces = []
            continue
        g = groups[t//FAR_GROUP]
        l1 = _clamp(max(g.a1, s.a1), s.a1, s.f1)
        l2 = min(max(g.g1, l1), s.f1)
        r2 = max(min(g.a2, s.a2), s.f2)
        r1 = max(min(g.g2, r2), s.f2)
        if mutation == "l1 and l2 swapped":
            l1, l2 = l2, l1
        # The four pieces in the order series_terms walks them.
        s.pieces = [(s.a1, l1), (l2, s.f1), (s.f2, r1), (r2, s.a2)]
        s.group_pieces = [(g.a1, g.g1), (g.g2, g.a2)]
        mark(t, s.a1, l1, TILE_COVER)
        mark(t, l2, s.f1, TILE_NEAR)
        mark(t, s.f2, r1, TILE_NEAR)
        mark(t, r2, s.a2, TILE_COVER)
        mark(t, max(g.a1, 0), max(g.g1, g.a1), GROUP)
        mark(t, g.g2, max(g.a2, g.g2), GROUP)
    return SimpleNamespace(case=case, tiling=tiling, farfield=farfield, level=lv, tiles=tiles,
                           groups=groups, classes=classes, count=count, nu=nu)


def pair_ratio(part, derived, tile, line):
    """rho = max |u|/|a| over the tile's points for a series pair: about the tile's centre, or
    about the group's centre for a line of the group's series."""
    s = part.tiles[tile]
    kind = part.classes[tile, line]
    centre = derived[line, 0]
    about = part.groups[tile//FAR_GROUP].centre if kind == GROUP else s.u0
    return max(abs(s.v_lo - about), abs(s.v_hi - about))/abs(centre - about)


def group_ratio(part, derived, group, line):
    g = part.groups[group]
    return max(abs(g.v_lo - g.centre), abs(g.v_hi - g.centre))/abs(derived[line, 0] - g.centre)


def partition_problems(part, derived):
    """What is wrong with a partition, judged by the window rule (spectra.c:48-62, as the oracle's
    derived first/last/status give it), by the far-wing limit of every line (voigt.c:34) and by
    the design ratio: an empty list for a right one."""
    problems = []
    n_lines = part.nu.size
    first, last, status = derived[:, 4], derived[:, 5], derived[:, 6]
    live = (status == 1.) & (last >= first)
    alpha, gamma = derived[:, 1], derived[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        repwid = np.sqrt(np.log(2.))/alpha
        y = repwid*gamma
        reach = np.where(y < 70.55, np.sqrt(np.maximum(15100. + y*(40. - y*3.6), 0.))/repwid, 0.)
    index = np.arange(n_lines)
    for t, s in enumerate(part.tiles):
        inside = (index >= s.lo) & (index < s.hi)
        if not np.array_equal(part.count[t], inside.astype(np.int32)):
            bad = np.flatnonzero(part.count[t] != inside)
            problems.append("tile %d: lines %s counted %s times" % (
                t, bad[:4].tolist(), part.count[t][bad[:4]].tolist()))
        overlaps = live & (first <= s.i1) & (last >= s.i0)
        covers = live & (first <= s.i0) & (last >= s.i1)
        kind = part.classes[t]
        if np.any(overlaps & (kind == OUTSIDE)):
            problems.append("tile %d: a window that overlaps it is outside" % t)
        whole = live & (kind != OUTSIDE) & (kind != CLIPPED)
        if np.any(whole & ~covers):
            problems.append("tile %d: line %d is summed unmasked, window [%d, %d]" % (
                t, np.flatnonzero(whole & ~covers)[0], first[np.flatnonzero(whole & ~covers)[0]],
                last[np.flatnonzero(whole & ~covers)[0]]))
        series = live & np.isin(kind, SERIES_CLASSES)
        for j in np.flatnonzero(series):
            distance = min(abs(derived[j, 0] - s.v_lo), abs(derived[j, 0] - s.v_hi))
            if not (s.v_lo > derived[j, 0] or s.v_hi < derived[j, 0]) or distance < reach[j]:
                problems.append("tile %d: line %d of the series has its core there" % (t, j))
            rho = pair_ratio(part, derived, t, j)
            if not rho <= 1./FAR_RATIO:
                problems.append("tile %d: line %d has rho = %.6f" % (t, j, rho))
    return problems


# ---------------------------------------------------------------------------------------------
# The series arithmetic (farfield.h, wave_ops.h, accumulate.h) in `dtype`.
def _line_terms(dtype, centre, g2, bl, u0):
    """[lines, FAR_TERMS]: q_k of every line about u0 (series_terms: add_line)."""
    a = dtype(1)*np.asarray(centre, dtype) - dtype(u0)
    r = dtype(1)/(a*a + np.asarray(g2, dtype))
    s = (a + a)*r
    q = np.zeros((a.size, FAR_TERMS), dtype)
    q[:, 0] = np.asarray(bl, dtype)*r
    q[:, 1] = s*q[:, 0]
    for k in range(2, FAR_TERMS):
        q[:, k] = s*q[:, k - 1] - r*q[:, k - 2]
    return q


def _threads_sum(dtype, terms, threads):
    """Line `at` of the list goes to thread at % threads, every thread adds its lines in order;
    then the 64 lanes of every wavefront as a balanced tree of neighbours, then the wavefronts
    as (0 + 1) + (2 + 3)."""
    rounds = -(-terms.shape[0]//threads) if terms.shape[0] else 0
    padded = np.zeros((max(rounds, 1)*threads, FAR_TERMS), dtype)
    padded[:terms.shape[0]] = terms
    padded = padded.reshape(-1, threads, FAR_TERMS)
    lanes = np.zeros((threads, FAR_TERMS), dtype)
    for m in range(padded.shape[0]):
        lanes = lanes + padded[m]
    waves = lanes.reshape(threads//64, 64, FAR_TERMS)
    while waves.shape[1] > 1:
        waves = waves[:, 0::2] + waves[:, 1::2]
    waves = waves[:, 0]
    if waves.shape[0] == 1:
        return waves[0]
    return (waves[0] + waves[1]) + (waves[2] + waves[3])


def series_coefficients(dtype, part, derived, tile, drop_last_taylor=False):
    """far_series[tile] of one level: the tile's own series plus the group's, re-centred."""
    s = part.tiles[tile]
    g = part.groups[tile//FAR_GROUP]
    live = (derived[:, 6] == 1.) & (derived[:, 5] >= derived[:, 4])
    # prepare_line: the record of a line without a window is mark_empty's (bl = 0).
    centre = np.where(live, derived[:, 0], 0.)
    g2 = np.where(live, derived[:, 2]*derived[:, 2], 1.)
    bl = np.where(live, derived[:, 3]*derived[:, 2]/np.pi, 0.)

    def listed(pieces):
        return np.concatenate([np.arange(a, max(b, a)) for a, b in pieces]).astype(np.int64)

    mine = listed(s.pieces)
    own = _threads_sum(dtype, _line_terms(dtype, centre[mine], g2[mine], bl[mine], s.u0), 64)
    theirs = listed(s.group_pieces)
    group_term = _threads_sum(dtype, _line_terms(dtype, centre[theirs], g2[theirs], bl[theirs],
                                                 g.centre), 256)
    d = dtype(s.u0 - g.centre)
    out = np.zeros(FAR_TERMS, dtype)
    for j in range(FAR_TERMS):
        shifted, weight = dtype(0), dtype(1)        # weight = C(j + m, j) d^m
        for m in range(FAR_TERMS - j):
            if not (drop_last_taylor and j + m == FAR_TERMS - 1):
                shifted = group_term[j + m]*weight + shifted
            weight = weight*(d*(dtype(j + m + 1)*(dtype(1)/dtype(m + 1))))
        out[j] = own[j] + shifted
    return out


def series_values(dtype, part, coefficients, tile):
    """Horner at every point of the tile (accumulate.h: series_at)."""
    s = part.tiles[tile]
    u = np.asarray(wavenumber(part.case, np.arange(s.i0, s.i1 + 1)), dtype) - dtype(s.u0)
    value = np.full(u.shape, coefficients[FAR_TERMS - 1], dtype)
    for k in range(FAR_TERMS - 2, -1, -1):
        value = value*u + coefficients[k]
    return value


def lorentz(case, derived, line, i0, i1):
    """S gamma/pi / ((v - c)^2 + gamma^2) at the grid points i0..i1 in long double."""
    ld = np.longdouble
    v = np.asarray(wavenumber(case, np.arange(i0, i1 + 1)), ld)
    centre, gamma, strength = (ld(derived[line, k]) for k in (0, 2, 3))
    d = v - centre
    return strength*gamma/ld(np.pi)/(d*d + gamma*gamma)


# ---------------------------------------------------------------------------------------------
# Tables.
def make_table(centres, delta_air=None, v0=1000):
    """Lines of one strength and one width (air and self alike), one isotopologue: no line of a
    table is hidden by another."""
    from pylbl_amd import synthetic
    centres = np.asarray(centres, dtype=np.float64)
    order = np.argsort(centres, kind="stable")
    n = centres.size
    table = synthetic.line_table("CO2", v0 - 30., v0 + 30., num_lines=n, seed=1,
                                 tips_range=(150, 400))
    table.nu = centres[order]
    table.sw = np.full(n, 1.e-21)
    table.gamma_air = np.full(n, 0.07)
    table.gamma_self = np.full(n, 0.07)
    table.n_air = np.full(n, 0.7)
    table.elower = np.full(n, 100.)
    table.delta_air = np.zeros(n) if delta_air is None else \
        np.asarray(delta_air, dtype=np.float64)[order]
    table.local_iso_id = np.ones(n, dtype=np.int32)
    return table


def handover_positions(case, lv, tiles=None, groups=None, ends=True):
    """(label, wavenumber, what, index, expected) of lines placed STEP beyond and STEP inside the
    far limits of tiles (first, middle, last by default) and groups (first and last) on either
    side, and STEP either side of cut_off + 1 outside either end of the grid."""
    tiling, farfield = call_tiling(case)
    out = []
    tiles = (0, tiling.n_tiles//2, tiling.n_tiles - 1) if tiles is None else tiles
    groups = (0, n_groups_of(tiling) - 1) if groups is None else groups
    for what, indices in (("tile", tiles), ("group", groups)):
        for index in indices:
            if what == "tile":
                i0, i1 = tile_bounds(tiling, index, case.npv, case.n)
            else:
                i0, i1 = group_bounds(case, tiling, index)
            centre, radius, _, _, _ = far_radius(lv, float(wavenumber(case, i0)),
                                                 float(wavenumber(case, i1)))
            for side, side_name in ((-1., "below"), (1., "above")):
                for sign, where in ((1., "beyond"), (-1., "inside")):
                    at = centre + side*(radius + lv.shift_max + sign*STEP)
                    out.append(("%s %d %s %s" % (what, index, side_name, where), at, what,
                                index, where))
    if ends:
        low, high = case.v0 - (case.cut_off + 1), case.vn + case.cut_off + 1
        for edge, name in ((low, "low end"), (high, "high end")):
            for sign, where in ((-1., "minus"), (1., "plus")):
                out.append(("%s %s" % (name, where), edge + sign*STEP, "end", 0, where))
        out.append(("last cell", float(case.vn + case.cut_off) - STEP, "end", 0, "inside"))
    return out


def table_for(case):
    """60 to 120 lines of one strength: hand-over lines of several tiles and groups (placed for
    the widest shift of FIVE_LEVELS), lines within 0.002 cm-1 of integers with pressure shifts up
    to +-0.02 cm-1/atm -- a third of the table, around the integers where the windows of the first
    and the last cells begin and end and across the grid -- and a uniform fill; no two centres
    closer than 0.02 cm-1, every line inside the range rule (absorption.c:80-83)."""
    low, high = case.v0 - (case.cut_off + 1), case.vn + case.cut_off + 1
    rng = np.random.default_rng(20 + case.cut_off + case.n)
    # The shifted lines first: the hand-over lines are placed for this table's shift_max.
    span = high - low
    integers = np.unique(np.round(np.linspace(low + 1, high - 1, min(30, span - 1)))).astype(int)
    near, delta = [], []
    for k, integer in enumerate(integers):
        offset = (0.001, -0.001, 0.0015, -0.0005)[k % 4]
        # Shifts that cross the integer at 1 atm and not at 10 Pa (against the offset), and shifts
        # that never do (with it).
        shift = (-0.02, 0.02, 0.012, 0.02, 0.02, -0.02, -0.015, -0.004)[k % 8]
        near.append(integer + offset)
        delta.append(shift)
    shifted = make_table(near, delta, case.v0)
    widest = max(level_scalars(shifted, t, p).shift_max for t, p in FIVE_LEVELS)
    lv = level_scalars(shifted, *FIVE_LEVELS[-1])
    lv.shift_max = widest
    tiling, _ = call_tiling(case)
    n_groups = n_groups_of(tiling)
    tiles = sorted({0, 1, tiling.n_tiles//2, tiling.n_tiles - 1})
    groups = sorted({0, n_groups//2, n_groups - 1})
    placed = [at for _, at, what, _, _ in handover_positions(case, lv, tiles, groups, ends=False)]
    # Just inside the range rule at either end.
    placed += [low + 0.3, high - 0.3]
    target = max(3*len(near), 60)
    fill = rng.uniform(low + 0.05, high - 0.05, 400)
    centres, deltas = list(near), list(delta)
    for at in placed + list(fill):
        if len(centres) >= target and at not in placed:
            break
        if low + 0.02 < at < high - 0.02 and np.min(np.abs(np.asarray(centres) - at)) >= 0.02 \
                and abs(at - round(at)) > 0.003:
            centres.append(at)
            deltas.append(0.)
    return make_table(centres, deltas, case.v0)
