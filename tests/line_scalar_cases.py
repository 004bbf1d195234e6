"""Inputs for the tests of the per-line scalars (csrc/line_prep.h: prepare_line, fed by fill_level
of csrc/lanes_plans.inc, run by prologue_kernel of csrc/tile_schedule.h or on the host with
prep = 1, returned in the reference's row order by derived_to_host of csrc/compute_stages.inc),
and two mirrors of that stage.

The float64 mirror restates fill_level and prepare_line up to `derived` in the reference's
operation order (spectra.c:17-62), nothing fused, exp and pow through the C library
(math.exp, math.pow), so that it can be held to the CPU oracle bit for bit.  The long-double
mirror continues from the SAME float64 level scalars (p_atm, p_partial, tfact, t_minus_ref,
t_times_ref, doppler[slot], q_ratio[slot]: the host forms them with correctly rounded operations)
and takes pow, the three exp and the products in numpy.longdouble.  The integer columns (first,
last, status) come from the float64 mirror alone.

Units of error per line, u = 2^-53:
    gamma      K_g = 1 + |n_air ln(tfact)|
    strength   K_s = 1 + |elower c2 (T - 296)/(T 296)| + 1/|1 - gg| + 1/|1 - gref|
(the condition numbers of pow, of the Boltzmann factor and of the two stimulated-emission
differences with respect to a rounding of their arguments; the quotient (1 - gg)/(1 - gref) loses
digits like T/(c2 nu) at small nu).  E_CPU_GAMMA and E_CPU_STRENGTH are the worst error of the
float64 mirror against the long-double mirror over every case below in these units
(tests/test_line_scalar_cases_host.py measures them and holds the records to the measurement); the
GPU tests allow (4 E_cpu + 1) u K.

Families: S isotopologue slots, E extremes, W windows, F shifts at the integer, R row order,
N line counts, B bad rows.
"""
from fractions import Fraction
from functools import lru_cache
import math
from types import SimpleNamespace

import numpy as np

from pylbl_amd.database import LineTable

U = 2.**-53
E_CAP = 8.                  # a condition on the units, not the bound
E_CPU_GAMMA = 2.94          # measured: tests/test_line_scalar_cases_host.py (2.933, family N)
E_CPU_STRENGTH = 1.68       # (1.675, family S)
MARGIN = 4.                 # device against host rounding (DESIGN.md sections 23, 27)

PA_TO_ATM = 9.86923e-6      # spectra.c:13
R2 = 2*math.log(2)*8314.472     # spectra.c:14
VLIGHT = 2.99792458e8
C2 = 1.4387752
MASS_SLOTS = 32             # line_prep.h: kMassSlots
INLINE_LEVELS = 4           # tile_schedule.h: kInlineLevels
NUM_ISO = 10
X = 4.e-4

COLUMNS = ("nu", "sw", "gamma_air", "gamma_self", "n_air", "elower", "delta_air")


class Refused(Exception):
    """fill_level refuses the level: T (or 296 K) outside the partition-function table."""


class BadRow(Exception):
    """An accepted row has no mass or no partition-function row (LBL_OUT_OF_RANGE)."""
    def __init__(self, row, local_iso_id):
        Exception.__init__(self, "row %d: local_iso_id %d" % (row, local_iso_id))
        self.row, self.local_iso_id = row, local_iso_id


# ---------------------------------------------------------------------------------------------
# Tables.
def slot_masses():
    return 20.*1.15**np.arange(NUM_ISO)


def tips(t_lo, t_hi):
    """Row s is q0_s (T/296)^(1.1 + 0.12 s): the ratio Q(296)/Q(T) differs by per cent from one
    isotopologue to the next, unlike the T^1.5 rows of every other table of the suite."""
    temperature = np.arange(float(t_lo), t_hi + 1., 1.)
    s = np.arange(NUM_ISO, dtype=np.float64)[:, None]
    return temperature, 100.*(1. + 0.37*s)*(temperature[None, :]/296.)**(1.1 + 0.12*s)


def make_table(columns, iso, tips_range=(100, 500), masses=None):
    """A LineTable of ten isotopologues (HITRAN ids 1..9 and 0, the tenth: slot 9) from a dict of
    the seven line columns, rows in the order given."""
    temperature, data = tips(*tips_range)
    fields = {x: np.ascontiguousarray(columns[x], dtype=np.float64) for x in COLUMNS}
    return LineTable(formula="XY", molecule_id=99,
                     local_iso_id=np.ascontiguousarray(iso, dtype=np.int32),
                     isoid=np.asarray(list(range(1, NUM_ISO)) + [0]),
                     mass=slot_masses() if masses is None else np.asarray(masses, np.float64),
                     tips_temperature=temperature, tips_data=data, **fields)


def random_columns(rng, nu):
    """Every row distinct in every column but (possibly) nu."""
    n = len(nu)
    return {"nu": np.asarray(nu, dtype=np.float64),
            "sw": 10.**rng.uniform(-26., -19., n),
            "gamma_air": rng.uniform(0.03, 0.12, n),
            "gamma_self": rng.uniform(0.05, 0.50, n),
            "n_air": rng.uniform(0.40, 0.85, n),
            "elower": rng.uniform(0., 3000., n),
            "delta_air": rng.uniform(-0.010, 0.002, n)}


def take(table, rows):
    """The rows `rows` of a table in that order."""
    rows = np.asarray(rows)
    return make_like(table, {x: getattr(table, x)[rows] for x in COLUMNS},
                     table.local_iso_id[rows])


def make_like(table, columns, iso):
    return LineTable(formula=table.formula, molecule_id=table.molecule_id,
                     local_iso_id=np.ascontiguousarray(iso, dtype=np.int32), isoid=table.isoid,
                     mass=table.mass, tips_temperature=table.tips_temperature,
                     tips_data=table.tips_data,
                     **{x: np.ascontiguousarray(columns[x], dtype=np.float64) for x in COLUMNS})


def _case(name, family, table, grid, levels, policies=("reference",), **more):
    """grid = (v0, vn, n_per_v, cut_off); levels = ((T, P, x), ...)."""
    v0, vn, npv, cut = grid
    assert (vn - v0 <= 32 and npv <= 10) or (vn - v0 <= 8 and npv <= 1000)
    assert table.num_lines <= 1300
    return SimpleNamespace(name=name, family=family, table=table, grid=grid, v0=v0, vn=vn,
                           npv=npv, cut_off=cut, n=(vn - v0)*npv, levels=tuple(levels),
                           policies=tuple(policies), **more)


GRID = (1000, 1032, 10, 25)

# -- S, slots ---------------------------------------------------------------------------------
S_IDS = tuple(range(11))        # 0 is HITRAN's tenth isotopologue (slot 9), like 10
S_LEVELS = ((296., 101325., X),     # Q(296)/Q(T) exactly 1
            (100., 5.e4, X),        # the first knot
            (250., 2.e4, 0.01),     # on a knot
            (250.5, 1.e3, 0.3),
            (499.999, 101325., X))  # the last interval: i + 1 = num_t - 1
S_REFUSED = ((99.99, 101325., X), (500., 101325., X))
S_NO_REFERENCE_LEVEL = (350., 101325., X)       # with a table on (300, 400): 296 K is missing


def s_table(tips_range=(100, 500)):
    rng = np.random.default_rng(101)
    n = 121
    nu = 980. + 72.*(np.arange(n) + 0.37)/n
    return make_table(random_columns(rng, nu), np.arange(n) % 11, tips_range)


# -- E, extremes ------------------------------------------------------------------------------
E_LEVELS = ((100., 0.5, 0.), (100., 1.2e5, 1.), (296., 101325., X), (899.25, 0.5, 1.),
            (220., 1.2e5, 0.), (899.25, 1.2e5, 0.5))


def e_table(centres):
    rows = [(nu, n_air, elower, gamma_self) for nu in centres
            for n_air in (-0.5, -0.1, 0., 0.7, 1.2) for elower in (0., 500., 12000.)
            for gamma_self in (0., 0.3)]
    rng = np.random.default_rng(102)
    columns = random_columns(rng, [r[0] for r in rows])
    columns["n_air"] = np.array([r[1] for r in rows])
    columns["elower"] = np.array([r[2] for r in rows])
    columns["gamma_self"] = np.array([r[3] for r in rows])
    columns["delta_air"] = 0.001*(np.arange(len(rows)) % 3 - 1.)
    return make_table(columns, (np.arange(len(rows)) + 1) % 11, (100, 900))


# -- W, windows -------------------------------------------------------------------------------
W_LEVEL = (296., 1.2e5, X)
W_P_ATM = 1.2e5*PA_TO_ATM
W_CUT_OFFS, W_NPV, W_V0 = (0, 1, 25), (1, 3, 10, 1000), (0, 10)
W_BRANCHES = ("first clamped", "left of the grid", "last is 0", "last clamped", "first is n - 1",
              "first is n", "first beyond n", "negative centre")

# Accepted rows per branch of W_BRANCHES, per case (tests/test_line_scalar_cases_host.py holds the
# mirror to them).  "first is n - 1" needs one point per cm-1: first is a multiple of n_per_v.
W_COUNTS = {
    (0, 1, 0): (3, 1, 2, 3, 3, 3, 2, 3), (0, 1, 10): (3, 2, 1, 3, 3, 3, 2, 0),
    (0, 3, 0): (3, 1, 2, 3, 0, 3, 2, 3), (0, 3, 10): (3, 2, 1, 3, 0, 3, 2, 0),
    (0, 10, 0): (3, 1, 2, 3, 0, 3, 2, 3), (0, 10, 10): (3, 2, 1, 3, 0, 3, 2, 0),
    (0, 1000, 0): (3, 1, 2, 3, 0, 3, 2, 3), (0, 1000, 10): (3, 2, 1, 3, 0, 3, 2, 0),
    (1, 1, 0): (5, 0, 1, 5, 2, 1, 2, 3), (1, 1, 10): (6, 2, 1, 5, 2, 1, 2, 0),
    (1, 3, 0): (5, 0, 1, 5, 0, 1, 2, 3), (1, 3, 10): (6, 2, 1, 5, 0, 1, 2, 0),
    (1, 10, 0): (5, 0, 1, 5, 0, 1, 2, 3), (1, 10, 10): (6, 2, 1, 5, 0, 1, 2, 0),
    (1, 1000, 0): (5, 0, 1, 5, 0, 1, 2, 3), (1, 1000, 10): (6, 2, 1, 5, 0, 1, 2, 0),
    (25, 1, 0): (7, 0, 0, 6, 1, 1, 2, 1), (25, 1, 10): (7, 0, 0, 6, 1, 1, 2, 1),
    (25, 3, 0): (7, 0, 0, 6, 0, 1, 2, 1), (25, 3, 10): (7, 0, 0, 6, 0, 1, 2, 1),
    (25, 10, 0): (7, 0, 0, 6, 0, 1, 2, 1), (25, 10, 10): (7, 0, 0, 6, 0, 1, 2, 1),
    (25, 1000, 0): (6, 0, 0, 7, 0, 1, 2, 1), (25, 1000, 10): (6, 0, 0, 7, 0, 1, 2, 1),
}       # key: (cut_off, n_per_v, v0)


def w_grid(cut_off, npv, v0):
    return (v0, v0 + (8 if npv == 1000 else 32), npv, cut_off)


def w_table(cut_off, npv, v0):
    """Lines whose floor(centre) = b sits at every edge of the window rule.  A b that no
    wavenumber >= 0 inside the range rule reaches is reached by a pressure shift of up to
    2.5 cm-1 from 0.3 cm-1 inside the rule's lower end, or left out."""
    v0, vn, npv, cut_off = w_grid(cut_off, npv, v0)
    nu_min, nu_max = v0 - (cut_off + 1), vn + cut_off + 1
    targets = [v0 - cut_off - 3, v0 - cut_off - 2, v0 - cut_off - 1, v0 - cut_off,
               v0 - cut_off + 1, v0, v0 + 1, (v0 + vn)//2, vn - cut_off - 2, vn - cut_off - 1,
               vn - cut_off, vn - 1, vn, vn + cut_off - 1, vn + cut_off, -1]
    nu, delta = [], []
    for b in targets:
        if b >= max(nu_min, 0) and b + 0.3 <= nu_max:
            nu.append(b + 0.3)
            delta.append(0.001)
        else:
            start = max(nu_min, 0) + 0.3
            shift = b + 0.2 - start
            if abs(shift) <= 2.5 and start <= nu_max:
                nu.append(start)
                delta.append(shift/W_P_ATM)
    # First beyond n: on the rule's upper end itself, and shifted over it.
    nu += [float(nu_max), nu_max - 0.2]
    delta += [0., 0.4/W_P_ATM]
    order = np.argsort(nu, kind="stable")
    rng = np.random.default_rng(103 + cut_off + npv + v0)
    columns = random_columns(rng, np.asarray(nu)[order])
    columns["delta_air"] = np.asarray(delta)[order]
    return make_table(columns, (np.arange(len(nu)) + 3) % 11)


# -- F, shifts at the integer -----------------------------------------------------------------
# (N, nu, delta_air) at P = 1.2e5 Pa: the float64 centre nu + fl(p_atm delta) is N or the double
# below N; "fused" is the correctly rounded p_atm delta + nu.  Found by a search in exact
# arithmetic (fractions.Fraction) over random shifts |p delta| <= 0.6.  Only one direction exists:
# the sum of the two doubles is a multiple of ulp(p delta), so it can lie ON the midpoint below N
# (and round to N, the even neighbour) with the exact product below it, never strictly under the
# midpoint with the exact sum at or over it.
F_LEVEL = (296., 1.2e5, X)
F_PAIRS = (
    (2, 1.8498854400743996, 0.12675301579218134),       # both N
    (2, 1.8498854400743994, 0.12675301579218134),       # both below
    (2, 1.5233434388365092, 0.4024769926018296),        # plain N, fused below
    (2, 1.5517358655244857, 0.37850313083823334),       # plain N, fused below
    (3, 3.5936816345213103, -0.5012900656225715),       # both N
    (3, 3.59368163452131, -0.5012900656225715),         # both below
    (3, 3.5955189095375086, -0.5028414151336265),       # plain N, fused below
    (3, 3.4190543769979573, -0.3538391352026767),       # plain N, fused below
    (10, 10.071623839374174, -0.06047739571558515),     # both N
    (10, 10.071623839374173, -0.06047739571558515),     # both below
    (10, 10.41872526630782, -0.35356124228859237),      # plain N, fused below
    (10, 9.912000738866654, 0.07430439620023134),       # plain N, fused below
    (1003, 1003.191918319095, -0.1620510744801369),     # both N
    (1003, 1003.1919183190948, -0.1620510744801369),    # both below
    (1003, 1002.9292601273258, 0.05973099613149168),    # plain N, fused below
    (1003, 1002.8766825704122, 0.1041261827482636),     # plain N, fused below
    (1016, 1016.3781499949944, -0.31930048831428653),   # both N
    (1016, 1016.3781499949943, -0.31930048831428653),   # both below
    (1016, 1015.7511298596223, 0.210139781571628),      # plain N, fused below
    (1016, 1015.8582018999285, 0.11973080310504815),    # plain N, fused below
    (1031, 1030.7958693915634, 0.1723628290797789),     # both N
    (1031, 1030.7958693915632, 0.1723628290797789),     # both below
    (1031, 1030.8178508855083, 0.15380220011389614),    # plain N, fused below
    (1031, 1031.507864471735, -0.4288281792121918),     # plain N, fused below
)
F_FUSED_DIFFER = {"F low": 6, "F high": 6}


def f_table(low):
    pairs = [p for p in F_PAIRS if (p[0] < 100) == low]
    order = np.argsort([p[1] for p in pairs], kind="stable")
    rng = np.random.default_rng(104)
    columns = random_columns(rng, np.asarray([p[1] for p in pairs])[order])
    columns["delta_air"] = np.asarray([p[2] for p in pairs])[order]
    return make_table(columns, (np.arange(len(pairs)) + 1) % 11)


def fused_centre(nu, delta, p_atm):
    """fma(p_atm, delta, nu) per line, in exact arithmetic."""
    return np.array([float(Fraction(p_atm)*Fraction(float(d)) + Fraction(float(v)))
                     for v, d in zip(nu, delta)])


# -- R, rows ----------------------------------------------------------------------------------
R_LEVEL = (260., 5.e4, 0.02)
R_OUTSIDE_AT = 24


def r_tables():
    """(R0, R): a permuted table with groups of equal nu, every row distinct in its other columns;
    R has a row outside the range rule in the middle, so that under the reference's policy the
    rows after it are never reached although in range."""
    rng = np.random.default_rng(105)
    nu = [1001.5]*4 + [1010.25]*3 + [1020.]*5 + list(np.round(rng.uniform(976., 1056., 36), 3))
    nu = np.asarray(nu)[rng.permutation(len(nu))]
    columns = random_columns(rng, nu)
    iso = rng.permutation(len(nu)) % 11
    r0 = make_table(columns, iso)
    with_outside = {x: np.insert(columns[x], R_OUTSIDE_AT, columns[x][0]) for x in COLUMNS}
    with_outside["nu"][R_OUTSIDE_AT] = 2000.
    with_outside["sw"][R_OUTSIDE_AT] = 3.e-22
    return r0, make_table(with_outside, np.insert(iso, R_OUTSIDE_AT, 2))


# -- N, counts --------------------------------------------------------------------------------
N_LINES = (1, 63, 64, 65, 255, 256, 257, 1025)      # wave and block edges of prepare_block
N_LEVEL = (240., 3.e4, X)


def n_table(n_lines):
    rng = np.random.default_rng(106 + n_lines)
    nu = np.sort(rng.uniform(975., 1057., n_lines))
    return make_table(random_columns(rng, nu), (np.arange(n_lines) + 5) % 11)


def empty_table():
    return make_table({x: np.zeros(0) for x in COLUMNS}, np.zeros(0, dtype=np.int32))


# -- B, bad rows ------------------------------------------------------------------------------
B_LEVEL = (280., 7.e4, X)
B_IDS = (11, -1, 33, 5)         # >= num_iso, below 1, beyond the 32 mass slots, and a mass of 0
B_GOOD_IDS = (1, 2, 3, 0, 10, 7)


def b_masses():
    masses = slot_masses()
    masses[4] = 0.
    return masses


def b_base():
    rng = np.random.default_rng(107)
    nu = rng.uniform(976., 1056., 30)       # not sorted: the engine sorts, and returns row order
    return make_table(random_columns(rng, nu), np.asarray(B_GOOD_IDS)[np.arange(30) % 6],
                      masses=b_masses())


B_OUT_AT = (3, 11, 19, 27)      # rows of the bad ids in B outside
B_IN_AT = 13                    # row of the bad id in B inside


def b_outside():
    base = b_base()
    columns = {x: getattr(base, x).copy() for x in COLUMNS}
    iso = base.local_iso_id.copy()
    for k, (row, bad) in enumerate(zip(B_OUT_AT, B_IDS)):
        columns["nu"][row] = (900., 1100.)[k % 2]
        iso[row] = bad
    return make_table(columns, iso, masses=b_masses())


def b_inside(bad):
    base = b_base()
    iso = base.local_iso_id.copy()
    iso[B_IN_AT] = bad
    return make_table({x: getattr(base, x) for x in COLUMNS}, iso, masses=b_masses())


# ---------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def cases():
    """name -> case: every (table, grid, levels, policies) the two test files walk."""
    out = []
    out.append(_case("S", "S", s_table(), GRID, S_LEVELS))
    out.append(_case("E low", "E", e_table((0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1., 3.7)),
                     (0, 8, 10, 25), E_LEVELS))
    out.append(_case("E high", "E", e_table((24990.5, 25000., 25000.25, 25010.75)),
                     (24996, 25004, 10, 25), E_LEVELS))
    for cut_off in W_CUT_OFFS:
        for npv in W_NPV:
            for v0 in W_V0:
                out.append(_case("W cut_off %d, %d per cm-1, v0 %d" % (cut_off, npv, v0), "W",
                                 w_table(cut_off, npv, v0), w_grid(cut_off, npv, v0), (W_LEVEL,)))
    out.append(_case("F low", "F", f_table(True), (0, 32, 10, 1), (F_LEVEL,)))
    out.append(_case("F high", "F", f_table(False), (1000, 1032, 10, 1), (F_LEVEL,)))
    r0, r = r_tables()
    out.append(_case("R0", "R", r0, GRID, (R_LEVEL,), ("reference", "skip")))
    out.append(_case("R", "R", r, GRID, (R_LEVEL,), ("reference", "skip")))
    for n_lines in N_LINES:
        out.append(_case("N %d" % n_lines, "N", n_table(n_lines), GRID, (N_LEVEL,)))
    out.append(_case("B outside", "B", b_outside(), GRID, (B_LEVEL,), ("reference", "skip")))
    return {c.name: c for c in out}


def walk():
    """(case, level, policy) of every call."""
    for case in cases().values():
        for level in case.levels:
            for policy in case.policies:
                yield case, level, policy


# ---------------------------------------------------------------------------------------------
# Mirrors.
def slots_of(table):
    """Slot per row, -1 for a row the engine can never evaluate (lbl_molecule_load)."""
    iso = np.asarray(table.local_iso_id, dtype=np.int64)
    slot = np.where(iso == 0, 10, iso) - 1          # spectral_database.c:173-177
    mass = table.mass_by_slot()
    num_iso = table.tips_data.shape[0]
    good = (slot >= 0) & (slot < MASS_SLOTS) & (slot < num_iso)
    good &= mass[np.clip(slot, 0, MASS_SLOTS - 1)] > 0.
    return np.where(good, slot, -1)


def tips_value(table, temperature, slot):
    """spectral_database.c:97-104 with fill_level's refusals."""
    t, q = table.tips_temperature, table.tips_data[slot]
    i = int(math.floor(temperature)) - int(t[0])
    if i < 0 or i + 1 >= t.size:
        raise Refused(temperature)
    return q[i] + (q[i + 1] - q[i])*(temperature - t[i])/(t[i + 1] - t[i])


def level_scalars(table, level):
    """LevelScalars of fill_level, in float64 and its order of operations."""
    temperature, pressure, vmr = (float(x) for x in level)
    p_atm = pressure*PA_TO_ATM
    lv = SimpleNamespace(temperature=temperature, p_atm=p_atm, p_partial=p_atm*vmr,
                         tfact=296./temperature, t_minus_ref=temperature - 296.,
                         t_times_ref=temperature*296., doppler=np.zeros(MASS_SLOTS),
                         q_ratio=np.zeros(MASS_SLOTS))
    mass = table.mass_by_slot()
    for slot in sorted(set(slots_of(table).tolist()) - {-1}):
        lv.doppler[slot] = math.sqrt(R2*temperature/mass[slot])
        lv.q_ratio[slot] = tips_value(table, 296., slot)/tips_value(table, temperature, slot)
    return lv


def accepted_rows(case, policy):
    """absorption.c:80-83 (the reference leaves its loop at the first row out of range), or
    every row in range; a row without a slot raises BadRow where it would be evaluated."""
    table = case.table
    nu = table.nu
    outside = (nu > case.vn + case.cut_off + 1) | (nu < case.v0 - (case.cut_off + 1))
    if policy == "reference":
        limit = int(np.flatnonzero(outside)[0]) if outside.any() else nu.size
        accepted = np.arange(nu.size) < limit
    else:
        accepted = ~outside
    bad = np.flatnonzero(accepted & (slots_of(table) < 0))
    if bad.size:
        raise BadRow(int(bad[0]), int(table.local_iso_id[bad[0]]))
    return accepted


def _windows(case, centre):
    """spectra.c:48-62 as prepare_line states it: (first, last, status) and, for the branch
    counts, the unclamped first and last."""
    fl = np.floor(centre)
    raw_first = np.trunc((fl - case.cut_off - float(case.v0))*case.npv).astype(np.int64)
    raw_last = np.trunc((fl + case.cut_off + 1 - float(case.v0))*case.npv).astype(np.int64)
    status = np.where(raw_first >= case.n, 0, 1)
    first = np.where(status == 1, np.maximum(raw_first, 0), raw_first)
    last = np.where(status == 1, np.minimum(raw_last, case.n - 1), 0)
    return first, last, status, raw_first, raw_last


def mirror64(case, level, policy, more=False):
    """derived[n_lines, 8] in the table's row order."""
    table = case.table
    lv = level_scalars(table, level)
    accepted = accepted_rows(case, policy)
    slot = np.maximum(slots_of(table), 0)
    nu = table.nu
    centre = nu + lv.p_atm*table.delta_air
    power = np.array([math.pow(lv.tfact, float(x)) for x in table.n_air])
    gamma = (table.gamma_air*(lv.p_atm - lv.p_partial) + table.gamma_self*lv.p_partial)*power
    alpha = (nu/VLIGHT)*lv.doppler[slot]
    exp = lambda x: np.array([math.exp(float(y)) for y in x])
    sb = exp(table.elower*C2*lv.t_minus_ref/lv.t_times_ref)
    gg = exp((-C2*nu)/lv.temperature)
    gref = exp((-C2*nu)/296.)
    se = (1. - gg)/(1. - gref)
    strength = table.sw*sb*se*lv.q_ratio[slot]*0.01*0.01
    first, last, status, raw_first, raw_last = _windows(case, centre)
    derived = np.zeros((nu.size, 8))
    derived[:, 6] = -1.
    for k, column in enumerate((centre, alpha, gamma, strength, first, last, status)):
        derived[accepted, k] = column[accepted]
    if more:
        return derived, SimpleNamespace(accepted=accepted, raw_first=raw_first, raw_last=raw_last,
                                        level=lv, slot=slot)
    return derived


def mirror_long(case, level, policy):
    """(gamma, strength, K_g, K_s) per row, the first two in long double from the float64 level
    scalars; NaN where the row is not accepted."""
    ld = np.longdouble
    table = case.table
    lv = level_scalars(table, level)
    accepted = accepted_rows(case, policy)
    slot = np.maximum(slots_of(table), 0)
    col = lambda x: np.asarray(getattr(table, x), dtype=ld)
    nu = col("nu")
    gamma = (col("gamma_air")*(ld(lv.p_atm) - ld(lv.p_partial)) +
             col("gamma_self")*ld(lv.p_partial))*np.power(ld(lv.tfact), col("n_air"))
    boltzmann = col("elower")*ld(C2)*ld(lv.t_minus_ref)/ld(lv.t_times_ref)
    gg = np.exp((-ld(C2)*nu)/ld(lv.temperature))
    gref = np.exp((-ld(C2)*nu)/ld(296.))
    se = (ld(1.) - gg)/(ld(1.) - gref)
    strength = col("sw")*np.exp(boltzmann)*se*np.asarray(lv.q_ratio[slot], ld)*ld(0.01)*ld(0.01)
    k_g = 1. + np.abs(table.n_air*math.log(lv.tfact))
    k_s = 1. + np.abs(boltzmann).astype(np.float64) + \
        (1./np.abs(1. - gg)).astype(np.float64) + (1./np.abs(1. - gref)).astype(np.float64)
    nan = ld(np.nan)
    return (np.where(accepted, gamma, nan), np.where(accepted, strength, nan),
            np.where(accepted, k_g, np.nan), np.where(accepted, k_s, np.nan))


def error_in_units(value, longer, k):
    """|value - longer|/(|longer| u K) per accepted row (0 where both are 0)."""
    ld = np.longdouble
    live = ~np.isnan(k)
    value, longer, k = np.asarray(value, ld)[live], longer[live], np.asarray(k, ld)[live]
    difference = np.abs(value - longer)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(difference == 0, ld(0.), difference/(np.abs(longer)*ld(U)*k))
    return out.astype(np.float64)


def bound_ratio(derived, case, level, policy):
    """(gamma, strength): the worst error of `derived` against the long-double mirror over the
    allowance (4 E_cpu + 1) u K of the GPU tests."""
    gamma, strength, k_g, k_s = mirror_long(case, level, policy)
    worst_g = error_in_units(derived[:, 2], gamma, k_g)
    worst_s = error_in_units(derived[:, 3], strength, k_s)
    return (float(np.max(worst_g, initial=0.))/(MARGIN*E_CPU_GAMMA + 1.),
            float(np.max(worst_s, initial=0.))/(MARGIN*E_CPU_STRENGTH + 1.))


def window_branches(case, level, policy="reference"):
    """How many accepted rows take each of W_BRANCHES."""
    derived, more = mirror64(case, level, policy, more=True)
    a = more.accepted
    first, last, status = derived[:, 4], derived[:, 5], derived[:, 6]
    n = case.n
    counts = (
        a & (status == 1) & (more.raw_first < 0),
        a & (status == 1) & (last < first),
        a & (status == 1) & (last == 0) & (last >= first),
        a & (status == 1) & (more.raw_last >= n),
        a & (status == 1) & (first == n - 1),
        a & (status == 0) & (more.raw_first == n),
        a & (status == 0) & (more.raw_first > n),
        a & (derived[:, 0] < 0),
    )
    return tuple(int(np.count_nonzero(c)) for c in counts)


def evals_of(derived):
    live = (derived[:, 6] == 1.) & (derived[:, 5] >= derived[:, 4])
    return int(np.sum(derived[live, 5] - derived[live, 4] + 1))


def oracle_derived(oracle, case, level, policy):
    """The CPU oracle's derived in row order; under the skip policy (which the reference does not
    have) its result on the rows in range, the others left as never reached."""
    table = case.table
    t, p, x = level
    if policy == "reference":
        rows = np.arange(table.num_lines)
    else:
        rows = np.flatnonzero(accepted_rows(case, policy))
    out = np.zeros((table.num_lines, 8))
    out[:, 6] = -1.
    _, extras = oracle.absorption_port(take(table, rows), t, p, x, case.v0, case.vn, case.npv,
                                       cut_off=case.cut_off, want_derived=True)
    out[rows] = extras["derived"]
    return out
