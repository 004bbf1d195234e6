"""lbl_solar_spectrum and lbl_path_solar fed directly (Engine.solar_spectrum / path_solar on rows held
in torch tensors) at the shapes Spectroscopy never gives them: sweep_cases' columns and layouts (odd
strides, bases that are not 16-byte aligned, NaN in the padding), depths 1, 8, 9, 16 and 17, both
orders, runs cut inside paths (LBL_PATH_CONTINUE and the carry rows), three paths under three Suns,
with and without a viewer, values chosen for the arithmetic, tables of 2 to 2^17 knots on
ascending, descending and shuffled grids, and calls that must be refused.
tests/test_solar_host.py proves on the CPU that the case tables of tests/solar_cases.py reach those
code paths.

Bounds, none taken from the code under test: the carry rows tau and tv are the float64 numpy loop
bit for bit; the space interface is F0 = mu0*S bit for bit; every other F and the reflected radiance
are within 1.2e-15 relative of the long-double F0*expl(-tau), resp. ((A*F0)/pi)*expl(-(tau + tv)),
formed from the float64 F0, quotient and optical depths (the suite's 1e-15 for exp plus one rounding
of the product), results below the smallest normal double within one subnormal step; band means
within 1e-12 * magnitude of the long-double means; the table within 6e-16*max(e_j, e_{j+1}) of the
long-double interpolation (five roundings, |e_{j+1} - e_j| <= max for values >= 0), a flat table
exact; the blackbody row within 1e-12 relative of the long-double scale*B."""
import numpy as np
import pytest

from tests import solar_cases as solar
from tests import sweep_cases as cases
from tests.test_gpu_sweep_shapes import (Rows, block, in_order, ordered, plain, read, same_bits,
                                         unfinished)

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
EXP_BOUND, MEAN_BOUND, TABLE_BOUND, PLANCK_BOUND = LD(1.2e-15), LD(1e-12), LD(6e-16), LD(1e-12)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def close(what, got, reference):
    """|got - reference| <= 1.2e-15*|reference|, one subnormal step where the reference is below
    the smallest normal double; never NaN or inf."""
    got, reference = np.asarray(got, dtype=F64), np.asarray(reference, dtype=LD)
    assert got.shape == reference.shape and got.size > 0, what
    assert np.all(np.isfinite(got)), what
    error = np.abs(got.astype(LD) - reference)
    allowed = np.where(np.abs(reference) < LD(solar.TINY), LD(solar.STEP),
                       EXP_BOUND*np.abs(reference))
    worst = float(np.max(error/np.maximum(allowed, LD(solar.STEP))))
    print("%s: worst error / bound %.3g" % (what, worst))
    assert np.all(error <= allowed), (what, worst)


def means_close(what, got, reference):
    """Band means of values >= 0 (their own magnitude): 1e-12 relative, NaN for empty bands."""
    got, reference = np.asarray(got, dtype=F64), np.asarray(reference, dtype=LD)
    assert got.shape == reference.shape, what
    empty = np.isnan(reference)
    assert np.array_equal(np.isnan(got), empty) and np.count_nonzero(~empty) > 0, what
    error = np.abs(got[~empty].astype(LD) - reference[~empty])
    assert np.all(error <= MEAN_BOUND*np.abs(reference[~empty])), what


# ---------------------------------------------------------------------------------------------
# lbl_path_solar.
def run_solar(engine, problem, layout, runs, from_last, view, mu0, s, lengths, albedo=None,
              albedo_rows=None, bands=None):
    """Every output of the sweep over `runs` (storage order; issued in the Sun's order)."""
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    solar_lengths, view_lengths = lengths
    beta = block(problem.beta, levels, columns, layout, np.nan)
    row = block(s[None, :], 1, columns, layout, np.nan)
    carry = block(None, 2*PATHS, columns, layout, SENTINEL)
    out_rows = {"interface_rows": block(None, levels, columns, layout, SENTINEL),
                "space_rows": block(None, PATHS, columns, layout, SENTINEL),
                "surface_rows": block(None, PATHS, columns, layout, SENTINEL)}
    keywords = {}
    if view:
        out_rows["reflected_rows"] = block(None, PATHS, columns, layout, SENTINEL)
        keywords["view_lengths"] = None
        if albedo_rows is not None:
            keywords["albedo_rows"] = Rows(block(albedo_rows, PATHS, columns, layout, np.nan))
        else:
            keywords["albedo"] = albedo
    means = {}
    if bands is not None:
        means = {name.replace("rows", "mean"): plain(rows.shape[0], bands.size - 1)
                 for name, rows in out_rows.items()}
    out = {}
    ordered(engine)
    for first, count in in_order(runs, from_last):
        part = slice(first, first + count)
        if view:
            keywords["view_lengths"] = view_lengths[part]
        per_level = {"interface_rows": Rows(out_rows["interface_rows"][part])}
        if bands is not None:
            per_level["interface_mean"] = Rows(means["interface_mean"][part])
        engine.path_solar(
            Rows(beta[part]), columns, PATHS, n, first, solar_lengths[part], mu0, Rows(row),
            Rows(carry), band_start=bands, from_last=from_last,
            **{k: Rows(v) for k, v in out_rows.items() if k != "interface_rows"},
            **{k: Rows(v) for k, v in means.items() if k != "interface_mean"},
            **per_level, **keywords)
        engine.synchronize()
        left = unfinished(first, count, n, from_last)
        if left is not None:
            both = read(carry, columns)
            out["tau@%d" % left[1]] = both[2*left[0]]
            if view:
                out["tv@%d" % left[1]] = both[2*left[0] + 1]
    out["carry"] = read(carry, columns).reshape(PATHS, 2, columns)
    out.update({name: read(rows, columns) for name, rows in out_rows.items()})
    out.update({name: read(rows) for name, rows in means.items()})
    assert np.array_equal(read(beta)[:, :columns], problem.beta), "beta was written"
    return out


def check_solar(what, problem, got, from_last, view, mu0, s, lengths, albedo=None, bands=None):
    n = problem.levels_per_path
    solar_lengths, view_lengths = lengths
    loop = solar.mirror(F64, problem, mu0, s, solar_lengths, from_last,
                        view_lengths if view else None, albedo)
    last = solar.last_rows(n, from_last)
    for key in got:
        if "@" in key:
            name, level = key.split("@")
            assert same_bits(got[key], loop[name][int(level)]), (what, key)
    assert same_bits(got["carry"][:, 0], loop["tau"][last]), (what, "tau")
    if view:
        assert same_bits(got["carry"][:, 1], loop["tv"][last]), (what, "tv")
    else:
        assert np.all(got["carry"][:, 1] == SENTINEL), (what, "tv was written without a viewer")
    assert same_bits(got["space_rows"], loop["f0"]), (what, "space")
    direct = solar.direct(LD, loop["f0"], loop["tau"], n)
    close((what, "direct"), got["interface_rows"], direct)
    assert same_bits(got["surface_rows"], got["interface_rows"][last]), (what, "surface")
    reference = {"interface": direct, "space": loop["f0"].astype(LD), "surface": direct[last]}
    if view:
        reference["reflected"] = solar.reflected(LD, loop["f0"], albedo, loop["tau"], loop["tv"],
                                                 n, from_last)
        close((what, "reflected"), got["reflected_rows"], reference["reflected"])
    if bands is not None:
        for name, values in reference.items():
            means_close((what, name + " mean"), got[name + "_mean"],
                        cases.band_means(LD, cases.flushed(values), bands))
    return loop


def standard(problem):
    return solar.MU0, solar.solar_row(problem), solar.lengths_of(problem)


@pytest.mark.parametrize("columns", cases.COLUMNS)
@pytest.mark.parametrize("view", [False, True])
def test_columns_layouts_and_a_viewer(engine, columns, view):
    """Every column count in the aligned layout, the layout columns in all five: the same bits."""
    problem = cases.Problem(columns, 9, seed=columns)
    mu0, s, lengths = standard(problem)
    layouts = list(cases.LAYOUTS) if columns in cases.LAYOUT_COLUMNS else ["aligned"]
    base = None
    for layout in layouts:
        got = run_solar(engine, problem, layout, [(0, problem.levels)], True, view, mu0, s,
                        lengths, solar.ALBEDO)
        if base is None:
            base = got
            check_solar((columns, layout), problem, got, True, view, mu0, s, lengths,
                        solar.ALBEDO)
        for key in base:
            assert same_bits(got[key], base[key]), (columns, layout, key)


@pytest.mark.parametrize("depth", solar.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_depths_and_both_orders(engine, depth, from_last):
    problem = cases.Problem(513, depth, seed=40 + depth)
    mu0, s, lengths = standard(problem)
    for layout in ("aligned", "odd"):
        got = run_solar(engine, problem, layout, [(0, problem.levels)], from_last, True, mu0, s,
                        lengths, solar.ALBEDO)
        check_solar((depth, from_last, layout), problem, got, from_last, True, mu0, s, lengths,
                    solar.ALBEDO)


@pytest.mark.parametrize("from_last", [False, True])
@pytest.mark.parametrize("view", [False, True])
def test_runs_cut_inside_paths_give_the_same_bits(engine, from_last, view):
    """Every run cut of sweep_cases for 3 x 19 levels: carry rows under LBL_PATH_CONTINUE."""
    problem = cases.Problem(131, solar.RUN_DEPTH, seed=9)
    mu0, s, lengths = standard(problem)
    rows = np.random.default_rng(2).uniform(0., 1., size=(PATHS, problem.columns))
    rows[0], rows[2, ::3] = 0.4, 0.
    base = None
    for name, runs in cases.run_sets(solar.RUN_DEPTH, cases.PATH_AHEAD).items():
        got = run_solar(engine, problem, "aligned", runs, from_last, view, mu0, s, lengths,
                        albedo_rows=rows)
        loop = check_solar((name, from_last), problem, got, from_last, view, mu0, s, lengths,
                           rows)
        if base is None:
            base = got
        for key in base:
            if "@" not in key:
                assert same_bits(got[key], base[key]), (name, key)
    assert loop is not None


@pytest.mark.parametrize("name, columns, bands", cases.BAND_SETS)
def test_band_means(engine, name, columns, bands):
    problem = cases.Problem(columns, 3, seed=70)
    mu0, s, lengths = standard(problem)
    whole = run_solar(engine, problem, "aligned", [(0, problem.levels)], True, True, mu0, s,
                      lengths, solar.ALBEDO, bands=bands)
    check_solar(name, problem, whole, True, True, mu0, s, lengths, solar.ALBEDO, bands=bands)
    cut = run_solar(engine, problem, "padded", [(0, 4), (4, 3), (7, 2)], True, True, mu0, s,
                    lengths, solar.ALBEDO, bands=bands)
    for key in whole:
        assert same_bits(cut[key], whole[key]), (name, key)


def test_values_chosen_for_the_arithmetic(engine):
    """beta = 0, of mixed sign and with tau > 745; S = 0 columns; mu0 = 1 and 1e-3; A = 0 and 1."""
    problem = solar.value_problem()
    lengths = (problem.solar_lengths, problem.view_lengths)
    group = problem.group
    for from_last in (False, True):
        got = run_solar(engine, problem, "padded", [(0, 5), (5, 13), (18, 9)], from_last, True,
                        problem.mu0, problem.solar, lengths, problem.albedo)
        loop = check_solar(("values", from_last), problem, got, from_last, True, problem.mu0,
                           problem.solar, lengths, problem.albedo)
        f0 = loop["f0"]
        level_path = solar.path_of_level(problem.levels_per_path)
        # beta = 0: F = F0 at every interface, bit for bit.
        assert same_bits(got["interface_rows"][:, group == 0], f0[level_path][:, group == 0])
        # tau > 745 underflows to 0, without NaN.
        assert np.all(got["surface_rows"][:, group == 1] == 0.)
        assert np.all(loop["tau"][solar.last_rows(9, from_last)][:, group == 1] > 745.)
        # S = 0 gives 0 whatever the optical depth, A = 0 gives no radiance, A = 1 F/pi's scale.
        dark = problem.solar == 0.
        assert np.any(dark) and np.all(got["interface_rows"][:, dark] == 0.)
        assert np.all(got["reflected_rows"][0] == 0.) and np.any(got["reflected_rows"][1] > 0.)
        assert np.any(loop["tau"] < 0.) and np.all(np.isfinite(got["interface_rows"]))


# ---------------------------------------------------------------------------------------------
# lbl_solar_spectrum.
def fill(engine, nu, layout="aligned", **keywords):
    grid = engine.load_grid(nu)
    try:
        row = block(None, 1, nu.size, layout, SENTINEL)
        ordered(engine)
        engine.solar_spectrum(grid, Rows(row), nu.size, **keywords)
        engine.synchronize()
        return read(row, nu.size)[0]
    finally:
        engine.free_grid(grid)


FILL_CASES = solar.fill_cases()


@pytest.mark.parametrize("name", sorted(FILL_CASES))
def test_table_matches_the_long_double_interpolation(engine, name):
    knots, nu = FILL_CASES[name]
    values = solar.table_values(knots)
    reference = solar.table(LD, knots, values, nu)
    j = np.clip(solar.interval(knots, nu), 0, knots.size - 2)
    allowed = TABLE_BOUND*np.maximum(values[j], values[j + 1]).astype(LD)
    for layout in ("aligned", "offset"):
        got = fill(engine, nu, layout, irradiance=values, wavenumber=knots)
        error = np.abs(got.astype(LD) - reference)
        print("%s, %s: worst error %.3g" % (name, layout, float(error.max())))
        assert np.all(error <= allowed), (name, layout)
        assert same_bits(got, solar.table(F64, knots, values, nu)), (name, layout)
    flat = fill(engine, nu, irradiance=np.full(knots.size, 0.7318), wavenumber=knots)
    assert np.all(flat == 0.7318), name
    scaled = fill(engine, nu, irradiance=values, wavenumber=knots, scale=1.0341)
    assert same_bits(scaled, solar.table(F64, knots, values, nu, 1.0341)), name


def test_blackbody_and_values_on_the_grid(engine):
    nu = np.concatenate([[-5., 0.], np.sort(np.random.default_rng(4).uniform(1., 40000., 1029))])
    scale = solar.SOLAR_SOLID_ANGLE*1.0334
    got = fill(engine, nu, temperature=solar.SOLAR_TEMPERATURE, scale=scale)
    reference = solar.blackbody(LD, nu, scale)
    assert np.all(got[:2] == 0.) and np.all(got[2:] > 0.)
    assert np.all(np.abs(got.astype(LD) - reference) <= PLANCK_BOUND*reference)
    values = np.random.default_rng(5).uniform(0., 2., size=nu.size)
    for layout in ("aligned", "offset"):
        assert same_bits(fill(engine, nu, layout, irradiance=values), values)
    assert same_bits(fill(engine, nu, irradiance=values, scale=0.967), 0.967*values)


# ---------------------------------------------------------------------------------------------
# Refused calls.
def test_rejected_calls_write_nothing(engine):
    from pylbl_amd.engine import EngineError
    problem = cases.Problem(67, 3, seed=1)
    mu0, s, (solar_lengths, view_lengths) = standard(problem)
    columns, levels = problem.columns, problem.levels

    def blocks():
        made = {"beta": block(problem.beta, levels, columns, "aligned", np.nan),
                "row": block(s[None, :], 1, columns, "aligned", np.nan)}
        for name, rows in (("carry", 2*PATHS), ("interface_rows", levels), ("space_rows", PATHS),
                           ("surface_rows", PATHS), ("reflected_rows", PATHS)):
            made[name] = block(None, rows, columns, "aligned", SENTINEL)
        return made

    good = dict(solar_lengths=solar_lengths, mu0=mu0, view_lengths=view_lengths,
                albedo=solar.ALBEDO, outputs=("interface_rows", "space_rows",
                                                 "surface_rows", "reflected_rows"))
    bad = [dict(solar_lengths=np.where(np.arange(levels) == 4, np.nan, solar_lengths)),
           dict(solar_lengths=-solar_lengths),
           dict(view_lengths=np.where(np.arange(levels) == 2, np.inf, view_lengths)),
           dict(mu0=np.array([1., 0., 0.5])), dict(mu0=np.array([1., 1.5, 0.5])),
           dict(mu0=np.array([1., np.nan, 0.5])),
           dict(albedo=None),                                   # a view without an albedo
           dict(albedo=np.array([0., 1.2, 0.5])),
           dict(view_lengths=None),                             # an albedo without a view
           dict(view_lengths=None, albedo=None),                # reflected rows without a view
           dict(outputs=("interface_rows", "space_rows")),      # a view without reflected rows
           dict(outputs=())]
    for change in bad:
        case = dict(good, **change)
        made = blocks()
        ordered(engine)
        with pytest.raises(EngineError, match="lbl_path_solar"):
            engine.path_solar(
                Rows(made["beta"]), columns, PATHS, 3, 0, case["solar_lengths"], case["mu0"],
                Rows(made["row"]), Rows(made["carry"]), view_lengths=case["view_lengths"],
                albedo=case["albedo"], **{name: Rows(made[name]) for name in case["outputs"]})
        engine.synchronize()
        for name in ("carry", "interface_rows", "space_rows", "surface_rows", "reflected_rows"):
            assert np.all(read(made[name]) == SENTINEL), (change, name)
    # The fill: bad tables, and the row stays as it was.
    nu = problem.nu
    grid = engine.load_grid(nu)
    row = block(None, 1, columns, "aligned", SENTINEL)
    for keywords in (dict(irradiance=[1., 2., 3.], wavenumber=[1., 1., 2.]),
                     dict(irradiance=[1., -2.], wavenumber=[1., 2.]),
                     dict(irradiance=[1., np.nan], wavenumber=[1., 2.]),
                     dict(irradiance=[1., 2.], wavenumber=[1., np.inf]),
                     dict(irradiance=[1.], wavenumber=[1.]),
                     dict(irradiance=np.ones(columns - 1)),
                     dict(temperature=0.), dict(temperature=5772., scale=0.),
                     dict(temperature=5772., scale=np.nan)):
        with pytest.raises(EngineError, match="lbl_solar_spectrum"):
            engine.solar_spectrum(grid, Rows(row), columns, **keywords)
    with pytest.raises(EngineError, match="lbl_solar_spectrum"):
        engine.solar_spectrum(grid + 1000, Rows(row), columns, temperature=5772.)
    engine.free_grid(grid)
    engine.synchronize()
    assert np.all(read(row) == SENTINEL)
