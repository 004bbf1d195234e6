"""Inputs for the tests of the scaled eights of the far-wing loop of accumulate_kernel<4>
(csrc/line_prep.h: WingGroup, wing_group_of; csrc/accumulate.h: aligned_share_of;
csrc/accumulate_lines.h: scaled_ranges; csrc/voigt_profile.h: scaled_eight), and a numpy mirror of

  * the group rule and the record's fields (group_record), bit for bit what lbl_wing_group gives;
  * the gate (a tile is eligible when its first point lies at or above max(64, 2 (cut_off + 2))
    cm-1, as an index rule) and the shares of an eligible tile (aligned_share_of): per (tile, part,
    wavefront) the aligned eights, which of them are scaled and which plain, and the ragged lines
    in front of and behind them, which go down the quads and left-overs of fast_ranges;
  * the arithmetic of a trip with exact rationals (fractions.Fraction, every fused multiply-add
    rounded once): scaled_eight, n = beta N, the running merge, the reciprocal left exact.

Tables are built eight by eight, so a case decides which lines share a table-aligned group.
Strengths are log-uniform over 1e-30 .. 1e-19 inside every ordinary eight, widths 1e-4 or 0.07.
"""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from tests import farfield_cases as fc
from tests import wing_share_cases as ws
from tests.inner_pass_cases import plan_parts, share_of

REACH = 1.5                 # line_prep.h: kWingGroupReach
SPREAD = 128                # line_prep.h: kWingGroupSpread
PLAIN_RECORD = np.array([0., 0., 1.]*8 + [0., 0.])
TINY = 2.2250738585072014e-308
HUGE = 1.7976931348623157e308


# ---------------------------------------------------------------------------------------------
# The group rule (line_prep.h).
def _normal(x):
    return TINY <= abs(x) <= HUGE


def group_beta(bl):
    mantissa, exponent = 1., 0
    for b in bl:
        m, e = np.frexp(b)
        mantissa *= float(m)
        exponent += int(e)
    q, r = exponent >> 3, exponent & 7
    return float(np.ldexp(np.sqrt(np.sqrt(np.sqrt(np.ldexp(mantissa, r)))), q))


def group_record(centre, g2, bl, lines=8):
    """(scaled, record[26]) of one table-aligned eight: eight times (s, nas, gs), beta, m."""
    centre, g2, bl = (np.asarray(x, dtype=np.float64) for x in (centre, g2, bl))
    if lines < 8 or not abs(centre[0]) < 4.e15:
        return False, PLAIN_RECORD.copy()
    if not all(b > 0. and _normal(b) for b in bl):
        return False, PLAIN_RECORD.copy()
    exponents = [int(np.frexp(b)[1]) - 1 for b in bl]
    if max(exponents) - min(exponents) > SPREAD:
        return False, PLAIN_RECORD.copy()
    beta = group_beta(bl)
    m = float(np.rint(centre[0]))
    if not _normal(beta):
        return False, PLAIN_RECORD.copy()
    record = np.zeros(26)
    with np.errstate(all="ignore"):
        for i in range(8):
            a = centre[i] - m
            s = float(np.sqrt(beta/bl[i]))
            nas = -(a*s)
            gs = g2[i]*(s*s)
            if not (abs(a) <= REACH and _normal(s) and _normal(gs) and abs(nas) <= HUGE):
                return False, PLAIN_RECORD.copy()
            record[3*i:3*i + 3] = (s, nas, gs)
    record[24], record[25] = beta, m
    return True, record


def library_record(centre, g2, bl, lines=8):
    from ctypes import c_void_p
    from pylbl_amd import abi
    lib = abi.library()
    arrays = [np.ascontiguousarray(x, dtype=np.float64) for x in (centre, g2, bl)]
    record = np.full(26, np.nan)
    status = lib.lbl_wing_group(*(c_void_p(a.ctypes.data) for a in arrays), int(lines),
                                c_void_p(record.ctypes.data))
    return status, record


def line_scalars(derived):
    """(centre, g2, bl, live) of every line from the oracle's derived columns, as prepare_line
    forms them; a line the engine marks empty has (0, 1, 0)."""
    centre, gamma, strength = derived[:, 0], derived[:, 2], derived[:, 3]
    live = (derived[:, 6] == 1.) & (derived[:, 5] >= derived[:, 4])
    return (np.where(live, centre, 0.), np.where(live, gamma*gamma, 1.),
            np.where(live, strength*gamma/np.pi, 0.), live)


def group_base(case, nu):
    """compute_stages.inc: wing_group_base -- the first line with nu >= v0 - (cut_off + 1)."""
    return int(np.searchsorted(nu, float(case.v0 - (case.cut_off + 1)), "left"))


def table_groups(derived, base=0):
    """[(scaled, record)] of every eight of a level, counted from line `base`."""
    centre, g2, bl, _ = line_scalars(derived)
    n = centre.size
    out = []
    for j in range(base, n, 8):
        lines = min(8, n - j)
        pad = lambda x, fill: np.concatenate([x[j:j + lines], np.full(8 - lines, fill)])
        out.append(group_record(pad(centre, 0.), pad(g2, 1.), pad(bl, 0.), lines))
    return out


# ---------------------------------------------------------------------------------------------
# Exact arithmetic.
def fma(a, b, c):
    """One rounding of a b + c (Fraction -> float is correctly rounded)."""
    return float(Fraction(a)*Fraction(b) + Fraction(c))


def scaled_eight(u, record):
    """voigt_profile.h: scaled_eight at u = v - m; (N, T)."""
    t = []
    for i in range(8):
        s, nas, gs = record[3*i:3*i + 3]
        d = fma(u, s, nas)
        t.append(fma(d, d, gs))
    big_n, big_t = fma(t[0], 1., t[1]), fma(t[0], t[1], 0.)
    for i in range(2, 8):
        big_n = fma(big_n, t[i], big_t)
        big_t = fma(big_t, t[i], 0.)
    return big_n, big_t


def trip(v, records):
    """accumulate_lines.h: scaled_ranges on one trip at one point; the quotient num/den exact."""
    num = den = None
    for record in records:
        big_n, t = scaled_eight(v - record[25], record)
        n = fma(record[24], big_n, 0.)
        if num is None:
            num, den = n, t
        else:
            num = fma(n, den, fma(num, t, 0.))
            den = fma(den, t, 0.)
    assert np.isfinite(num) and np.isfinite(den) and 2.**-300 < den < 2.**300
    return Fraction(num)/Fraction(den)


def exact_sum(v, centre, g2, bl):
    return sum(Fraction(b)/((Fraction(v) - Fraction(c))**2 + Fraction(g)) for c, g, b in
               zip(centre, g2, bl))


# ---------------------------------------------------------------------------------------------
# Cases.
STANDARD = ws.LEVEL
# (T = 296 K throughout: S(T) = sw without an exponential, so the host's and the device's line
# scalars are the same numbers whatever their exp() do in the last bit)
COLD = (296., 2000., 4.e-4)


def _case(name, v0, span, cut_off, eights, tail=(), levels=(STANDARD,), points=4, caps=(8,),
          unsorted=(), accumulate=False, scale_density=False):
    """`eights`: a list of groups, each up to eight (nu, sw, width) in table order; `tail`: lines
    after the last whole group; `unsorted`: rows appended in the reference's row order that sort
    elsewhere (a row out of range, then the rows the range rule refuses)."""
    return SimpleNamespace(name=name, v0=v0, vn=v0 + span, npv=1000, n=span*1000, points=points,
                           cut_off=cut_off, eights=eights, tail=tuple(tail), levels=tuple(levels),
                           caps=tuple(caps), unsorted=tuple(unsorted), accumulate=accumulate,
                           scale_density=scale_density, farfield=0, aligned=0)


def _strengths(rng, count=8):
    return 10.**rng.uniform(-30., -19., count)


def _filled(rng, lo, hi, n_eights, widths=(1.e-4, 0.07)):
    """`n_eights` ordinary eights over [lo, hi): centres increasing, each group within 1.4 cm-1 of
    its first line's nearest integer."""
    edges = np.linspace(lo, hi, n_eights + 1)
    out = []
    for g in range(n_eights):
        a, b = edges[g], min(edges[g + 1], edges[g] + 0.9)
        nu = np.sort(rng.uniform(a, b, 8)) if b - a > 1.e-6 else a + 1.e-7*np.arange(8)
        width = widths[g % len(widths)]
        out.append([(float(x), float(s), width) for x, s in zip(nu, _strengths(rng))])
    return out


def _special_eights(rng, at):
    """Plain groups of every kind and their scaled neighbours, from `at` (an integer) upwards."""
    ulp = np.spacing(at + 5.5)
    def eight(first, last, first_exact=None):
        nu = np.sort(rng.uniform(first, last, 8))
        nu[0], nu[-1] = first, last
        if first_exact is not None:
            nu[0] = first_exact
        return [(float(x), float(s), 0.07) for x, s in zip(nu, _strengths(rng))]
    out = []
    # an eight spanning just under and just over 1.5 cm-1 from m
    out.append(eight(at + 0.01, at + 1.4999))                  # m = at
    out.append(eight(at + 1.51, at + 3.5001))                  # m = at + 2
    # a first line at x.5 -/+ 1 ulp: m = at + 4 and at + 6
    out.append(eight(at + 4.5 - ulp, at + 4.9, first_exact=at + 4.5 - ulp))
    out.append(eight(at + 5.0, at + 5.4))
    out.append(eight(at + 5.5 + ulp, at + 6.2, first_exact=at + 5.5 + ulp))
    # one negative amplitude
    group = eight(at + 6.3, at + 6.9)
    group[3] = (group[3][0], -1.e-28, 0.07)
    out.append(group)
    out.append(eight(at + 7.0, at + 7.6))
    return out


def _cases():
    out = {}
    rng = np.random.default_rng(20240607)
    # Both sides of the 64 cm-1 gate, cut-off 2 (inner_everywhere); cold, narrow lines.
    out["gate-64"] = _case("tiles on both sides of the 64 cm-1 gate, cut-off 2", 60, 10, 2,
                           _filled(rng, 57.2, 72.8, 40), levels=(COLD,), caps=(2, 8))
    # Cut-off 25 around 2500: every kind of plain group in the middle of a trip.
    eights = _filled(rng, 2470.2, 2488., 14) + _special_eights(rng, 2488) + \
        _filled(rng, 2496.0, 2527.5, 20)
    refused = 2512.345
    out["cut-25"] = _case(
        "cut-off 25 around 2500, plain groups of every kind", 2495, 8, 25, eights,
        tail=[(2527.6 + 0.1*i, 1.e-22, 0.07) for i in range(3)],
        unsorted=[(2495 + 8 + 25 + 5., 1.e-22, 0.07), (refused, 1.e-20, 0.07)],
        caps=(2, 4, 8), accumulate=True, scale_density=True)
    # Cut-off 40: the gate is 2 (40 + 2) = 84, inside the grid.
    out["cut-40"] = _case("cut-off 40: the gate at 84 cm-1", 80, 8, 40,
                          _filled(rng, 41.2, 126.5, 36), levels=(COLD,))
    # Thirteen lines: the left range is exactly one aligned eight, the right one shorter than one.
    out["sparse"] = _case("a range of one eight and one shorter than an eight", 1000, 6, 25,
                          [[(990. + 0.15*i, 1.e-21, 0.07) for i in range(8)]],
                          tail=[(1011. + 0.5*i, 1.e-21, 0.07) for i in range(5)])
    # Parts 2, 5 and the cap of 64 (plan_for: 128 lines per item on these grids).
    out["parts-2"] = _case("parts 2, three lines below the window", 1200, 6, 25,
                           _filled(rng, 1176., 1230., 26),
                           unsorted=[(1170.1 + 0.1*i, 1.e-20, 0.07) for i in range(3)])
    out["parts-5"] = _case("parts 5", 1200, 6, 25, _filled(rng, 1176., 1230., 72))
    out["parts-64"] = _case("parts 64, the cap", 1200, 6, 25, _filled(rng, 1176., 1230., 1100))
    # K = 4, 2, 1: one eight of very weak lines lowers the level's bound on |bl|.
    for k, weak in ((4, 1.e-240), (2, 1.e-270), (1, 1.e-290)):
        eights = _filled(rng, 2470.2, 2494., 20) + \
            [[(2494.2 + 0.05*i, weak, 0.07) for i in range(8)]] + _filled(rng, 2495.2, 2527.5, 20)
        out["K-%d" % k] = _case("K = %d" % k, 2495, 6, 25, eights, caps=(2, 4, 8))
    # Two levels of one call with different K: the weak eight is narrow, so its |bl| follows the
    # pressure.
    eights = _filled(rng, 2470.2, 2494., 20) + \
        [[(2494.2 + 0.05*i, 1.e-255, 0.07) for i in range(8)]] + _filled(rng, 2495.2, 2527.5, 20)
    out["two-levels"] = _case("two levels, K differs", 2495, 6, 25, eights,
                              levels=(STANDARD, (296., 1.e-3, 4.e-4)))
    # The other kernels: the old loop.
    for p in (1, 2, 8):
        out["P%d" % p] = _case("points_per_lane %d" % p, 2495, 6, 25,
                               _filled(rng, 2470.2, 2527.5, 30), points=p)
    return out


CASES = _cases()
EXPECTED_K = {"K-4": 4, "K-2": 2, "K-1": 1, "parts-5": 8}


def make_table(case):
    lines = [l for group in case.eights for l in group] + list(case.tail)
    sorted_nu = np.array([l[0] for l in lines])
    assert np.all(np.diff(sorted_nu) > 0.), case.name
    lines += list(case.unsorted)
    n = len(lines)
    table = ws._blank_table(case, n)
    table.nu = np.array([l[0] for l in lines])
    table.sw = np.array([l[1] for l in lines])
    table.gamma_air = np.array([l[2] for l in lines])
    table.gamma_self = np.array([l[2] for l in lines])
    return table


class Runs(object):
    """key -> case, table, per level the oracle's spectrum and derived scalars in SORTED order;
    made on first use, kept and never written to."""

    def __init__(self, oracle):
        self.oracle, self.kept = oracle, {}

    def __call__(self, key):
        if key not in self.kept:
            case = CASES[key]
            table = make_table(case)
            order = np.argsort(table.nu, kind="stable")
            k_ref, derived = [], []
            for level in case.levels:
                k, extras = self.oracle.absorption_port(table, *level, case.v0, case.vn, case.npv,
                                                        cut_off=case.cut_off, want_derived=True)
                k.setflags(write=False)
                k_ref.append(k)
                derived.append(extras["derived"][order])
            self.kept[key] = SimpleNamespace(case=case, table=table, k_ref=k_ref, derived=derived,
                                             nu=np.asarray(table.nu)[order])
        return self.kept[key]


# ---------------------------------------------------------------------------------------------
# The mirror of the shares.
def gate_index(case):
    """compute_stages.inc: AccumulateArgs::scaled_from."""
    gate = max(64, 2*(case.cut_off + 2))
    return max(0, gate - case.v0)*case.npv


def aligned_share_of(j0, j1, part, parts, base=0):
    """accumulate.h: aligned_share_of -> (s0, s1, r0, r1)."""
    first = base + ((max(j0, base) - base + 7) & ~7)
    last = base + ((j1 - base) & ~7) if j1 > base else first
    if first >= last:
        return first, first, j0, (j1 if part == 0 else j0)
    s0, s1 = share_of(first, last, part, parts, 3)
    if part + 1 == parts:
        return s0, s1, last, j1
    return s0, s1, j0, (first if part == 0 else j0)


def walk(case, s, piece, pieces, scaled_flags, points, base=0):
    """What one wavefront does with the far-wing ranges of tile `s`: `eligible`, the line indices
    that ride scaled eights, plain eights, quads (fast_ranges) and left-overs (general_line)."""
    eligible = points == 4 and s.i0 >= gate_index(case)
    scaled, plain, ragged = [], [], []
    if eligible:
        for j0, j1 in ((s.f1, s.c1), (s.c2, s.f2)):
            s0, s1, r0, r1 = aligned_share_of(j0, j1, piece, pieces, base)
            for j in range(s0, s1, 8):
                (scaled if scaled_flags[(j - base) >> 3] else plain).append(j)
            ragged.append((r0, r1))
    else:
        ragged = [share_of(s.f1, s.c1, piece, pieces, 2), share_of(s.c2, s.f2, piece, pieces, 2)]
    quads, left = [], []
    for r0, r1 in ragged:
        quads += list(range(r0, r0 + ((r1 - r0) & ~3)))
        left += list(range(r0 + ((r1 - r0) & ~3), r1))
    eights_lines = [j + i for j in scaled + plain for i in range(8)]
    return SimpleNamespace(eligible=eligible, scaled=scaled, plain=plain, quads=quads, left=left,
                           ragged=ragged, walked=sorted(eights_lines + quads + left))


def mirror(run, level=0):
    """{(tile, part, wave): walk} of one level and the schedule of every tile."""
    case = run.case
    tiling = fc.pick_tiling(case.points, 0, case.npv, case.n)
    lv = fc.level_scalars(run.table, *case.levels[level][:2])
    base = group_base(case, run.nu)
    flags = [scaled for scaled, _ in table_groups(run.derived[level], base)]
    parts, _, _ = plan_parts(case, tiling, run.nu)
    schedules, walks = {}, {}
    for t in range(tiling.n_tiles):
        s = fc.schedule_tile(case, tiling, 0, run.nu, lv, t)
        if s.hi == s.lo:
            continue
        schedules[t] = s
        pieces = int(parts[t])*4
        for piece in range(pieces):
            walks[(t, piece >> 2, piece & 3)] = walk(case, s, piece, pieces, flags, tiling.p, base)
    return SimpleNamespace(case=case, tiling=tiling, parts=parts, schedules=schedules,
                           walks=walks, flags=flags, base=base)
