"""The running merge of the far-wing loop (accumulate_lines.h: fast_ranges<4>) with its carried
sums near the ends of their range.  A trip of K batches carries N and T = prod t from batch to
batch -- N = n T + (N t), T = T t, the product N t rounded on its own -- and line_prep.h
(wing_batches) picks K per level so that both stay normal.  tests/test_gpu_wing_batches.py and
tests/test_gpu_wing_shares.py pin the loop at strengths of 1e-30 ... 1e-19; here the strengths of
five of the former's cases reach down to 1e-45, which lowers the smallest amplitude by fifty
binary orders, brings N that much nearer to the lower guard n t_lo + b_lo >= -1000, and takes
one case across it.

Shapes: points_per_lane = 4, a grid of 2 cm-1 at 1000 points per cm-1 (eight tiles of 256
points), the line counts of the cases (600 and 2500).  Every case runs under both draws.

    case                       t_lo  t_hi   b_lo (1e-30 / 1e-45)    K (1e-30 / 1e-45)
    narrow lines near 1 cm-1   -34     3    -157 / -207             2 / 2    (16 t_lo + b_lo = -751)
    narrow lines near 2 cm-1   -34     3    -157 / -206             2 / 2
    narrow lines near 3 cm-1   -26     3    -156 / -205             4 / 2    (32 t_lo = -832: -988 holds,
                                                                              -1037 does not)
    cut-off 180                -10    15    -126 / -175             8 / 8    (64 t_hi + 6 = 966)
    cut-off 181                -10    16    -126 / -176             4 / 4    (64 t_hi + 6 = 1030)

On grids of fewer than 1024 tiles lanes_plans.inc (plan_for) cuts a tile into items of at most 128
lines, 32 per wavefront: the longest trip of these shapes is four batches (the cut-off cases), three
and two in the narrow ones -- test_the_cases_reach_their_trips states it from the mirror of
tests/wing_share_cases.py.  Trips of eight batches are run by tests/test_gpu_wing_shares.py
(batch-long, 1025 tiles).

Bounds, none from the kernel's output: against the CPU oracle zero exactly where it is zero,
tests/wing_share_cases.rounding_bound(N) relative where N lines cover the point, every value
finite; two runs give the same bits; every cap of wing_batches at or above the level's K gives
the bits of the uncapped run; a cap of K/4, where K >= 4, gives another spectrum.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import wing_share_cases as ws
from tests.test_gpu_wing_batches import CASES, case_table, expected_batches

NPV, SPAN, POINTS = 1000, 2, 4
WEAKEST = {"1e-30": -30., "1e-45": -45.}
# label -> K under the draw of tests/test_gpu_wing_batches.py and under the redrawn strengths,
# and the longest trip (in batches) a wavefront walks at that K.
EXPECTED = {
    "narrow lines near 1 cm-1": {"1e-30": (2, 2), "1e-45": (2, 2)},
    "narrow lines near 2 cm-1": {"1e-30": (2, 2), "1e-45": (2, 2)},
    "narrow lines near 3 cm-1": {"1e-30": (4, 3), "1e-45": (2, 2)},
    "cut-off 180": {"1e-30": (8, 4), "1e-45": (8, 4)},
    "cut-off 181": {"1e-30": (4, 4), "1e-45": (4, 4)},
}
KEYS = [(label, draw) for label in EXPECTED for draw in WEAKEST]
IDS = ["%s, sw from %s" % key for key in KEYS]


class Runs(object):
    """(label, draw) -> case, table, K, reference and bound, made once and never written to."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.kept = {}

    def __call__(self, key):
        if key not in self.kept:
            label, draw = key
            _, formula, v0, _, _, cut, t, p, x, lines, _ = next(c for c in CASES if c[0] == label)
            vn = v0 + SPAN
            table = case_table(label, formula, v0, vn, cut, lines)
            rng = np.random.default_rng(len(label))
            table.sw = rng.permutation(10.**np.linspace(WEAKEST[draw], -19., table.nu.size))
            case = SimpleNamespace(name="%s, sw from %s" % key, tile=0, v0=v0, vn=vn, npv=NPV,
                                   n=SPAN*NPV, points=POINTS, cut_off=cut, farfield=0, aligned=0,
                                   levels=((t, p, x),))
            k_ref, extras = self.oracle.absorption_port(table, t, p, x, v0, vn, NPV, cut_off=cut,
                                                        want_derived=True)
            k_ref.setflags(write=False)
            covering = ws.lines_covering(case, extras["derived"])
            bound = np.array([ws.rounding_bound(n) for n in range(int(covering.max()) + 1)])
            batches = expected_batches(self.oracle, table, t, p, x, v0, vn, NPV, cut)
            self.kept[key] = SimpleNamespace(case=case, table=table, batches=batches, k_ref=[k_ref],
                                             derived=[extras["derived"]], bound=bound[covering])
        return self.kept[key]


@pytest.fixture(scope="module")
def runs(oracle):
    return Runs(oracle)


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_the_cases_reach_their_batches(runs, key):
    """lbl_wing_batches on the bounds of the case: both sides of the lower guard."""
    assert runs(key).batches == EXPECTED[key[0]][key[1]][0]


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_the_cases_reach_their_trips(runs, key):
    """Some wavefront carries its sums over more than one batch, as far as the plan lets it."""
    run = runs(key)
    walks = ws.mirror(run, 0, run.batches).walks.values()
    assert max(max(wing.trips, default=0) for wing, _ in walks) == EXPECTED[key[0]][key[1]][1]
    assert max(wing.eights for wing, _ in walks) <= 4


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_merged_trips_at_the_ends_of_their_range(engine, runs, key):
    run = runs(key)
    case, want = run.case, run.batches
    (t, p, x), = case.levels
    engine.set_option("points_per_lane", POINTS)
    molecule = engine.load(run.table)
    try:
        def spectrum(cap):
            engine.set_option("wing_batches", cap)
            return engine.compute(molecule, np.array([t]), np.array([p]), np.array([x]), case.v0,
                                  case.vn, case.npv, cut_off=case.cut_off)[0].copy()
        k = spectrum(8)
        k_ref = run.k_ref[0]
        zero = k_ref == 0
        error = np.zeros(case.n)
        with np.errstate(invalid="ignore", divide="ignore"):
            error[~zero] = np.abs(k[~zero] - k_ref[~zero])/np.abs(k_ref[~zero])
        print("%s: K = %d, worst relative difference %.3g, %.3g x the bound" % (
            case.name, want, float(np.nanmax(error)), float(np.nanmax(error/run.bound))))
        assert np.all(np.isfinite(k)), case.name
        assert np.array_equal(k[zero], k_ref[zero]), case.name
        assert np.all(error <= run.bound), case.name
        assert np.array_equal(spectrum(8), k), case.name
        for cap in (1, 2, 4, 8):
            if cap >= want:
                assert np.array_equal(spectrum(cap), k), (case.name, cap)
        if want >= 4:
            assert not np.array_equal(spectrum(want//4), k), case.name
    finally:
        engine.free(molecule)
        engine.set_option("wing_batches", 8)
        engine.set_option("points_per_lane", 0)
