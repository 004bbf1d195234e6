"""The core range of the accumulate kernel evaluates a 64-point row of a line as one quotient in
(v - centre)^2 -- far wing or w4 region 1 from the constants A, B, A2 of the line record -- and
merges two lines per reciprocal; rows on which a lane has a selection to make take the reference's
chain (accumulate_lines.h: core_pair, general_line).  Small tables whose lines sit where those
paths part, at every tile size, with and without the far-field series, against the CPU oracle.

Bounds: the contract (1e-6); with the series off 1e-12 relative at every non-zero point (the
quotient form, the merge and the Newton reciprocal are each good to ~1e-15; dropping the 1/r^2
term of A or B, the smallest mistake the form allows, moves values by >= 3e-5); with the series
on its truncation level, 1e-9."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1.e-6             # the contract (tests/test_gpu_parity.py)
ROUNDING = 1.e-12       # series off
SERIES = 1.e-9          # series on (tests/test_gpu_api.py)

V0, VN, NPV = 1000, 1002, 1000
T, P, X = 296., 101325., 4.e-4

# y = repwid*gamma, and why (voigt.c).
Y_VALUES = (5.e-7,      # w4 avoided, voigt.c:48-53
            1.e-3,      # small-y region 1
            0.5, 0.9,   # B = 2 g2 - 1/r^2 changes sign at y = 1/sqrt(2)
            5.,         # mid range
            8.42,       # xlim1 small
            8.43,       # xlim1 = 0: region 1 through the centre
            30.,        # large y
            71.)        # pure Lorentz branch, voigt.c:17-27

# Centres [cm-1] on the grid 1000-1002 at 1000 points per cm-1 (index = (nu - 1000)*1000).  Plain
# tiles are 64 P points (boundaries at multiples of 64 P), the series' tiles divide the 1 cm-1
# cells (boundaries at 1000.5, 1001.0, ...).
MID = 1000.700          # mid-tile at P = 8 and 4, either tiling
EDGE = 1000.512         # boundary of the plain tiles of every P
EDGE_CELL = 1001.000    # boundary of the cell-aligned tiles
ROW_IN = 1000.576       # one row (64 points) from a plain tile boundary
NEAR = 1000.710         # 0.01 from MID: the pair has the same class on every row
OUT_FAR = 999.700       # 0.3 outside the grid
OUT_NEAR = 999.950      # 0.05 outside: the grid begins in its region 1
# A wavefront takes a quarter of the lines whose cores may reach its tile and walks them two at a
# time: a pair forms only where eight or more lines lie within a line's reach (0.137 cm-1 here) of
# one tile.  The lines of "eight" and "nine" all do for the 64-point tile that begins at ROW_IN
# (and so for the wider tiles that hold it), "nine" with a line left over; in the smaller tables
# every line is walked alone.  pair_kinds() checks both from the inputs.
TABLES = {
    "one": (MID,),
    "pair-near": (MID, NEAR),
    "pair-apart": (MID, EDGE_CELL),             # 0.3 apart: different classes on the same row
    "three": (OUT_FAR, OUT_NEAR, EDGE_CELL),
    "eight": (EDGE, ROW_IN, 1000.600, 1000.640, 1000.660, MID, NEAR, 1000.740),
    "nine": (EDGE, ROW_IN, 1000.600, 1000.640, 1000.660, 1000.680, MID, NEAR, 1000.740),
}
CONFIGS = [(points, farfield) for points in (1, 2, 4, 8) for farfield in (0, 1)]


def make_table(centres, y, oracle):
    """Lines at `centres` whose y = repwid*gamma is `y` at (T, P): no shift, no temperature
    exponent, one isotopologue, air and self widths equal, so gamma = width*p_atm."""
    from pylbl_amd import synthetic
    n = len(centres)
    table = synthetic.line_table("CO2", 999., 1003., num_lines=n, seed=1, tips_range=(150, 400))
    table.nu = np.asarray(sorted(centres), dtype=np.float64)
    table.sw = np.geomspace(3.e-21, 1.e-22, n)
    table.n_air = np.zeros(n)
    table.elower = np.full(n, 100.)
    table.delta_air = np.zeros(n)
    table.local_iso_id = np.ones(n, dtype=np.int32)
    table.gamma_air = np.full(n, 0.07)
    table.gamma_self = np.full(n, 0.07)
    _, extras = oracle.absorption_port(table, T, P, X, V0, VN, NPV, want_derived=True)
    alpha = extras["derived"][:, 1]
    width = y*alpha/np.sqrt(np.log(2.))/(P*9.86923e-6)
    table.gamma_air = width.copy()
    table.gamma_self = width.copy()
    return table


def line_limits(table, oracle):
    """(centre, repwid, xlim0, xlim1) per line from the oracle's scalars (voigt.c:13-14, :34-53);
    xlim0 = 0 marks the pure Lorentz branch (every point far wing)."""
    _, extras = oracle.absorption_port(table, T, P, X, V0, VN, NPV, want_derived=True)
    d = extras["derived"]
    out = []
    for centre, alpha, gamma in d[:, :3]:
        repwid = np.sqrt(np.log(2.))/alpha
        y = repwid*gamma
        if y >= 70.55:
            out.append((centre, repwid, 0., 0., y))
            continue
        xlim0 = np.sqrt(15100. + y*(40. - y*3.6))
        xlim1 = 0. if y >= 8.425 else np.sqrt(164. - y*(4.3 + y*1.8))
        if y <= 0.000001:
            xlim1 = xlim0
        out.append((centre, repwid, xlim0, xlim1, y))
    return out


def tile_rows(points, farfield, npv, n):
    """[first, last] of every 64-point row of every tile (lanes_plans.inc: pick_tiling with a
    forced P; accumulate.h: tile_bounds)."""
    width = 64*points
    per_cell = -(-npv//width)
    rows = []
    if farfield and per_cell*width/npv - 1. <= 0.06:
        length = -(-npv//per_cell)
        for cell in range(n//npv):
            for sub in range(per_cell):
                i0 = cell*npv + sub*length
                i1 = min(i0 + length - 1, (cell + 1)*npv - 1, n - 1)
                rows += [(r, min(r + 63, i1)) for r in range(i0, i1 + 1, 64)]
    else:
        for i0 in range(0, n, width):
            i1 = min(i0 + width - 1, n - 1)
            rows += [(r, min(r + 63, i1)) for r in range(i0, i1 + 1, 64)]
    return rows


def row_classes(limits, rows, npv):
    """Which kinds of (line, row) occur: decided on the inputs alone."""
    seen = set()
    for centre, repwid, xlim0, xlim1, _ in limits:
        for first, last in rows:
            v = V0 + np.arange(first, last + 1)*(1./npv)
            abx = np.abs((v - centre)*repwid)
            far = abx >= xlim0
            one = ~far & (abx >= xlim1)
            inner = ~far & ~one
            if far.all():
                seen.add("far")
            elif one.all():
                seen.add("region 1")
            else:
                if far.any():
                    seen.add("straddles xlim0")
                if inner.any() and one.any():
                    seen.add("straddles xlim1")
    return seen


def row_kind(limit, first, last, npv):
    centre, repwid, xlim0, xlim1, _ = limit
    abx = np.abs((V0 + np.arange(first, last + 1)*(1./npv) - centre)*repwid)
    if (abx >= xlim0).all():
        return "far"
    if ((abx < xlim0) & (abx >= xlim1)).all():
        return "region 1"
    return "chain"


def pair_kinds(limits, points, farfield, npv):
    """Most lines whose reach (xlim0/repwid) meets one tile, and the kinds of rows that two
    neighbours of the sorted table have together on the tiles both reach: what core_pair can be
    handed.  From the inputs alone."""
    rows = tile_rows(points, farfield, npv, (VN - V0)*npv)
    tiles, start = [], 0
    for k, (first, last) in enumerate(rows):
        if k + 1 == len(rows) or rows[k + 1][0] != last + 1 or (k + 1 - start) == points:
            tiles.append(rows[start:k + 1])
            start = k + 1
    most, kinds = 0, set()
    for tile in tiles:
        lo, hi = V0 + tile[0][0]/npv, V0 + tile[-1][1]/npv
        inside = [l for l in limits if l[2] > 0. and lo - l[2]/l[1] <= l[0] <= hi + l[2]/l[1]]
        most = max(most, len(inside))
        for a, b in zip(inside[:-1], inside[1:]):
            for first, last in tile:
                ka, kb = row_kind(a, first, last, npv), row_kind(b, first, last, npv)
                if "chain" in (ka, kb):
                    kinds.add("chain + chain" if ka == kb else "chain + quotient")
                else:
                    kinds.add(ka + " + " + kb if ka == kb else "mixed")
    return most, kinds


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(oracle):
    """(name, y) -> (table, reference spectrum, limits): made once, never written to."""
    out = {}
    for name, centres in TABLES.items():
        for y in Y_VALUES:
            table = make_table(centres, y, oracle)
            k_ref, _ = oracle.absorption_port(table, T, P, X, V0, VN, NPV)
            k_ref.setflags(write=False)
            out[(name, y)] = (table, k_ref, line_limits(table, oracle))
    return out


def test_the_widths_give_the_y_values(cases):
    for (name, y), (_, _, limits) in cases.items():
        for _, _, xlim0, xlim1, got in limits:
            assert abs(got - y) <= 1.e-5*y, (name, y, got)
            if y == 5.e-7:
                assert got <= 0.000001 and xlim1 == xlim0
            if y == 8.42:
                assert got < 8.425 and 0. < xlim1 < 1.
            if y == 8.43:
                assert got >= 8.425 and xlim1 == 0.
            if y == 71.:
                assert got >= 70.55


def worst_relative(k, k_ref):
    nz = k_ref != 0
    assert np.array_equal(k[~nz], k_ref[~nz]), "non-zero where the reference is zero"
    return float(np.max(np.abs(k[nz] - k_ref[nz])/np.abs(k_ref[nz]))) if nz.any() else 0.


@pytest.mark.parametrize("points,farfield", CONFIGS)
def test_tables_against_the_oracle(engine, cases, points, farfield):
    rows = tile_rows(points, farfield, NPV, (VN - V0)*NPV)
    seen = set()
    # What core_pair is handed, from the inputs: eight lines or more on one tile, and among sorted
    # neighbours rows of every kind.  (A 64-point tile is one row, and a line that reaches it is
    # not in the far wing on it: far rows need P >= 2, and a far row beside a region-1 row is
    # looked for in either tiling of this P.)
    most, kinds, either = 0, set(), set()
    for name in ("eight", "nine"):
        for y in Y_VALUES:
            n, k = pair_kinds(cases[(name, y)][2], points, farfield, NPV)
            most, kinds = max(most, n), kinds | k
            either |= k | pair_kinds(cases[(name, y)][2], points, 1 - farfield, NPV)[1]
    assert most >= 8, most
    assert kinds >= {"region 1 + region 1", "chain + quotient", "chain + chain"}, kinds
    if points >= 2:
        assert "far + far" in kinds and "mixed" in either, (kinds, either)
    engine.set_option("points_per_lane", points)
    engine.set_option("farfield", farfield)
    try:
        for (name, y), (table, k_ref, limits) in cases.items():
            seen |= row_classes(limits, rows, NPV)
            molecule = engine.load(table)
            try:
                k = engine.compute(molecule, T, P, X, V0, VN, NPV)[0].copy()
                again = engine.compute(molecule, T, P, X, V0, VN, NPV)[0].copy()
            finally:
                engine.free(molecule)
            label = f"{name} y={y:g} P={points} farfield={farfield}"
            assert np.array_equal(k, again), label
            worst = worst_relative(k, k_ref)
            print(f"{label}: worst relative difference {worst:.3g}")
            assert worst <= REL, label
            assert worst <= (SERIES if farfield else ROUNDING), label
    finally:
        engine.set_option("points_per_lane", 0)
        engine.set_option("farfield", 0)
    assert seen == {"far", "region 1", "straddles xlim0", "straddles xlim1"}, seen


@pytest.mark.parametrize("points", [1, 2, 4, 8])
def test_a_table_is_the_sum_of_its_lines(engine, cases, points):
    """The two-line tables, and "eight", whose lines are walked in pairs."""
    engine.set_option("points_per_lane", points)
    try:
        for name in ("pair-near", "pair-apart", "eight"):
            for y in Y_VALUES:
                table = cases[(name, y)][0]
                n = table.num_lines
                spectra = []
                for keep in [np.ones(n, bool)] + [np.arange(n) == j for j in range(n)]:
                    molecule = engine.load(table.subset(keep))
                    try:
                        spectra.append(engine.compute(molecule, T, P, X, V0, VN, NPV)[0].copy())
                    finally:
                        engine.free(molecule)
                together, alone = spectra[0], np.sum(spectra[1:], axis=0)
                worst = float(np.max(np.abs(together - alone)/alone))
                print(f"{name} y={y:g} P={points}: table against sum {worst:.3g}")
                assert worst <= ROUNDING, (name, y, points)
    finally:
        engine.set_option("points_per_lane", 0)


def test_host_and_device_records_agree(engine, cases):
    table, k_ref, _ = cases[("nine", 0.9)]
    molecule = engine.load(table)
    try:
        results = []
        for prep in (0, 1):
            engine.set_option("prep", prep)
            results.append(engine.compute(molecule, T, P, X, V0, VN, NPV)[0].copy())
    finally:
        engine.set_option("prep", 0)
        engine.free(molecule)
    assert np.array_equal(results[0], results[1])
    assert worst_relative(results[1], k_ref) <= ROUNDING


def test_two_thousand_points_per_wavenumber(engine, oracle):
    table = make_table(TABLES["nine"], 0.5, oracle)
    k_ref, _ = oracle.absorption_port(table, T, P, X, V0, VN, 2000)
    limits = line_limits(table, oracle)
    for points, farfield in ((8, 0), (8, 1)):
        rows = tile_rows(points, farfield, 2000, (VN - V0)*2000)
        assert row_classes(limits, rows, 2000) == {"far", "region 1", "straddles xlim0",
                                                   "straddles xlim1"}
    molecule = engine.load(table)
    try:
        for farfield, bound in ((0, ROUNDING), (1, SERIES)):
            engine.set_option("farfield", farfield)
            k = engine.compute(molecule, T, P, X, V0, VN, 2000)[0].copy()
            worst = worst_relative(k, k_ref)
            print(f"2000 points per cm-1, farfield={farfield}: {worst:.3g}")
            assert worst <= min(bound, REL)
    finally:
        engine.set_option("farfield", 0)
        engine.free(molecule)


def test_with_the_pedestal_removed(engine, cases, oracle):
    from tests import golden_io
    table, k_plain, _ = cases[("nine", 5.)]
    k_ref, _ = oracle.absorption_port(table, T, P, X, V0, VN, NPV, remove_pedestal=True)
    molecule = engine.load(table)
    try:
        k = engine.compute(molecule, T, P, X, V0, VN, NPV, remove_pedestal=True)[0].copy()
    finally:
        engine.free(molecule)
    tol = np.maximum(golden_io.pedestal_tolerance(k_ref, NPV, 25, REL), REL*np.abs(k_plain))
    worst = float(np.max(np.abs(k - k_ref)/(tol + 1e-300)))
    print(f"pedestal removed: {worst:.3g} x the pedestal tolerance")
    assert worst <= 1.
