"""lbl_path_two_stream_spectral and lbl_path_thermal_two_stream_spectral fed directly (Engine's
path_two_stream_spectral and path_thermal_two_stream_spectral on rows held in torch tensors) on
the case tables of tests/scatterer_cases.py: sweep_cases' layout columns, the depths 1, 8, 9 and 17
(every loop of path_levels with the 4, 2 and 1 rows in flight of the spectral kernels), both storage
orders, M = 2, 3 and 1024 knots, knots between the two columns of a lane, between two lanes and on
grid points, grid points below and above all knots, descending grids, levels without a scatterer,
with one that only absorbs, with one that scatters at some knots only, and tau_c that falls to
exactly 0 at a knot with grid points one ulp either side of it; the longwave entry with both
sources.  tests/test_scatterer_host.py proves on the CPU that the tables hold these.

Bounds, none taken from the code under test.  The reference is the long-double mirror of
tests/scatterer_cases.py -- the interpolation and its limit in float64, then the layers and adding
of tests/two_stream_cases.py, tests/thermal_cases.py and tests/thermal_source_cases.py, continued
from the float64 layer inputs.  Every flux is within (4*E_cpu + 1e-13)*scale of it: scale = F0 and
E_cpu = 1.03e-11 (recorded as scatterer_cases.E_CPU_SHORTWAVE = 1.1e-11) for the shortwave entry,
scale = pi*max B and E_cpu = 2.69e-15 (E_CPU_LONGWAVE = 3e-15) for the longwave one, the worst
|float64 mirror - long-double mirror|/scale that tests/test_scatterer_host.py measures over the same
tables, capped at 1e-10; the factor 4 and the floor as in tests/test_gpu_two_stream_shapes.py and
tests/test_gpu_thermal_shapes.py.  A flat table gives the grey entry's bits.  Where every
temperature of a path is the same the linear source gives the bits of the level-temperature source.
Nothing is NaN or inf.  Aligned and odd layouts (the vector and the scalar kernels), and one run
against one run per path, give identical bits."""
import numpy as np
import pytest

from tests import scatterer_cases as sc
from tests import sweep_cases as cases
from tests import thermal_source_cases as tsc
from tests.test_gpu_sweep_shapes import Grid, Rows, block, ordered, read, same_bits

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
SHORTWAVE_BOUND = LD(4.*sc.E_CPU_SHORTWAVE + sc.FLUX_FLOOR)
LONGWAVE_BOUND = LD(4.*sc.E_CPU_LONGWAVE + sc.FLUX_FLOOR)
SHORTWAVE_NAMES = tuple(prefix + q for prefix in ("", "top_") for q in sc.ts.QUANTITIES)
LONGWAVE_NAMES = sc.tc.NAMES
SHORTWAVE_CASES, LONGWAVE_CASES = sc.shortwave_cases(), sc.longwave_cases()


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def whole(inputs):
    return [(0, inputs.levels)]


def per_path(inputs, reverse=False):
    n = inputs.levels_per_path
    runs = [(p*n, n) for p in range(PATHS)]
    return runs[::-1] if reverse else runs


def _outputs(names, inputs, layout):
    return {name: block(None, PATHS if name.startswith("top_") else inputs.levels,
                        inputs.columns, layout, SENTINEL) for name in names}


def _collect(inputs, beta, work, rows):
    out = {name: read(tensor, inputs.columns) for name, tensor in rows.items()}
    out["work"] = read(work, inputs.columns)
    assert np.array_equal(read(beta)[:, :inputs.columns], inputs.beta), "beta was written"
    return out


def shortwave(engine, inputs, layout, runs, from_last, grey=None, knots=None, optics=None):
    """Every output of lbl_path_two_stream_spectral over `runs` of whole paths (first level,
    count); with `grey` (a two_stream_cases.Inputs) of lbl_path_two_stream on that table."""
    n, columns, levels = inputs.levels_per_path, inputs.columns, inputs.levels
    knots = inputs.knots if knots is None else knots
    optics = inputs.optics if optics is None else optics
    beta = block(inputs.beta, levels, columns, layout, np.nan)
    solar = block(inputs.solar[None, :], 1, columns, layout, np.nan)
    sigma = block(inputs.sigma[None, :], 1, columns, layout, np.nan)
    work = block(None, 2*levels, columns, layout, SENTINEL)
    rows = _outputs(SHORTWAVE_NAMES, inputs, layout)
    keywords = {}
    if inputs.albedo.ndim == 2:
        keywords["albedo_rows"] = Rows(block(inputs.albedo, PATHS, columns, layout, np.nan))
    else:
        keywords["albedo"] = inputs.albedo
    with Grid(engine, inputs.nu) as grid:
        ordered(engine)
        for first, count in runs:
            part = slice(first, first + count)
            outputs = {name + "_rows": Rows(rows[name] if name.startswith("top_")
                                            else rows[name][part]) for name in rows}
            tail = (inputs.mu0, Rows(solar), Rows(work[2*first:2*(first + count)]))
            if grey is not None:
                engine.path_two_stream(Rows(beta[part]), columns, PATHS, n, first,
                                       grey.table[part], *tail, rayleigh_row=Rows(sigma),
                                       from_last=from_last, **outputs, **keywords)
            else:
                engine.path_two_stream_spectral(
                    Rows(beta[part]), columns, grid, PATHS, n, first, inputs.table[part], knots,
                    optics[part], *tail, rayleigh_row=Rows(sigma), from_last=from_last, **outputs,
                    **keywords)
            engine.synchronize()
    return _collect(inputs, beta, work, rows)


def longwave(engine, inputs, layout, runs, from_last, linear, grey=None, knots=None,
             optics=None):
    """Every output of lbl_path_thermal_two_stream_spectral with either source; with `grey` (a
    thermal_source_cases.Inputs) of the grey entry of that source on that table."""
    n, columns, levels = inputs.levels_per_path, inputs.columns, inputs.levels
    knots = inputs.knots if knots is None else knots
    optics = inputs.optics if optics is None else optics
    beta = block(inputs.beta, levels, columns, layout, np.nan)
    work = block(None, 2*levels, columns, layout, SENTINEL)
    rows = _outputs(LONGWAVE_NAMES, inputs, layout)
    keywords = {}
    if inputs.emissivity.ndim == 2:
        keywords["emissivity_rows"] = Rows(block(inputs.emissivity, PATHS, columns, layout, np.nan))
    else:
        keywords["emissivity"] = inputs.emissivity
    with Grid(engine, inputs.nu) as grid:
        ordered(engine)
        for first, count in runs:
            part = slice(first, first + count)
            outputs = {name + "_rows": Rows(rows[name] if name.startswith("top_")
                                            else rows[name][part]) for name in rows}
            common = dict(diffusivity=inputs.diffusivity, from_last=from_last)
            head = (Rows(beta[part]), columns, grid, PATHS, n, first)
            tail = (inputs.surface_t, Rows(work[2*first:2*(first + count)]))
            if grey is None:
                engine.path_thermal_two_stream_spectral(
                    *head, inputs.table[part], knots, optics[part], *tail,
                    edge_temperature=inputs.edges[part] if linear else None, **common, **outputs,
                    **keywords)
            elif linear:
                engine.path_thermal_two_stream_source(*head, grey.table[part], grey.edges[part],
                                                      *tail, **common, **outputs, **keywords)
            else:
                engine.path_thermal_two_stream(*head, grey.table[part], *tail, **common,
                                               **outputs, **keywords)
            engine.synchronize()
    return _collect(inputs, beta, work, rows)


def close(what, names, got, reference, top, bound):
    """Every flux within bound*scale of the long-double mirror (top [PATHS, columns]: the scale
    at interface 0; a path's levels share it), and finite."""
    scale = {True: top.astype(LD), False: np.repeat(top, got[names[0]].shape[0]//PATHS,
                                                    axis=0).astype(LD)}
    for name in names:
        value = got[name]
        assert np.all(np.isfinite(value)), (what, name)
        error = np.abs(value.astype(LD) - reference[name])
        allowed = bound*scale[name.startswith("top_")]
        lit = allowed > 0.
        worst = float(np.max(error[lit]/allowed[lit], initial=0.))
        print("%s, %s: worst error / bound %.3g" % (what, name, worst))
        assert np.all(error <= allowed), (what, name, worst)
    assert np.all(np.isfinite(got["work"])), (what, "work")


def same(what, got, base):
    for key in base:
        assert same_bits(got[key], base[key]), (what, key)


# ---------------------------------------------------------------------------------------------
# The case tables.
@pytest.mark.parametrize("index", range(len(SHORTWAVE_CASES)))
def test_shortwave_case_tables_match_the_mirror(engine, index):
    inputs, from_last = SHORTWAVE_CASES[index]
    what = (inputs.name, from_last)
    got = shortwave(engine, inputs, "aligned", whole(inputs), from_last)
    reference = sc.shortwave_mirror(LD, inputs, from_last)
    close(what, SHORTWAVE_NAMES, got, reference, reference["f0"], SHORTWAVE_BOUND)
    assert same_bits(got["top_direct"], reference["f0"]), (what, "F0")
    assert np.all(got["top_diffuse"] == 0.), (what, "diffuse light from space")
    # The scalar kernels on an odd stride, one run per path: the same bits.
    same(what, shortwave(engine, inputs, "odd", per_path(inputs, from_last), from_last), got)


@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("index", range(len(LONGWAVE_CASES)))
def test_longwave_case_tables_match_the_mirror(engine, index, linear):
    inputs, from_last = LONGWAVE_CASES[index]
    what = (inputs.name, from_last, "linear" if linear else "isothermal")
    got = longwave(engine, inputs, "aligned", whole(inputs), from_last, linear)
    reference = sc.longwave_mirror(LD, inputs, from_last, linear)
    close(what, LONGWAVE_NAMES, got, reference, reference["scale"], LONGWAVE_BOUND)
    assert np.all(got["top_down"] == 0.), (what, "light from space")
    first = inputs.order(from_last)[:, 0]
    assert same_bits(got["top_up"], got["work"][2*first]), (what, "U[0]")
    same(what, longwave(engine, inputs, "odd", per_path(inputs, from_last), from_last, linear),
         got)


@pytest.mark.parametrize("index", [3, 9, 14])
def test_equal_temperatures_give_the_linear_source_the_isothermal_bits(engine, index):
    """Path 2 of every longwave table has one temperature at every interface and level: with
    spectral optics too the linear source's outputs are the level-temperature source's."""
    inputs, from_last = LONGWAVE_CASES[index]
    assert np.all(inputs.interfaces[2] == tsc.EQUAL_T)
    assert np.all(inputs.table[2*inputs.levels_per_path:, 4] == tsc.EQUAL_T)
    n = inputs.levels_per_path
    linear = longwave(engine, inputs, "aligned", whole(inputs), from_last, True)
    plain = longwave(engine, inputs, "aligned", whole(inputs), from_last, False)
    for name in LONGWAVE_NAMES:
        part = slice(2, 3) if name.startswith("top_") else slice(2*n, 3*n)
        assert same_bits(linear[name][part], plain[name][part]), (inputs.name, name)
    assert same_bits(linear["work"][4*n:], plain["work"][4*n:]), (inputs.name, "work")
    # (The other paths have temperatures that differ, and fluxes that do.)
    assert not same_bits(linear["up"][:2*n], plain["up"][:2*n]), inputs.name


# ---------------------------------------------------------------------------------------------
# Flat tables.
def level_optics(inputs):
    """[levels, 3]: a grey scatterer out of the table's first knot; every fourth level only
    absorbs, every fifth has none."""
    level = inputs.optics[:, 0, :].copy()
    level[::4, 1] = 0.
    level[::5, 0] = 0.
    return level


@pytest.mark.parametrize("m", [2, 5, sc.MAX_KNOTS])
@pytest.mark.parametrize("from_last", [False, True])
def test_a_flat_table_gives_the_grey_entries_bits(engine, m, from_last):
    knots = np.sort(np.random.default_rng(m).uniform(-50., 3200., size=m))
    inputs = sc.shortwave_inputs(513, 9, 3, 11, albedo_rows=True)
    level = level_optics(inputs)
    flat = sc.flat_optics(level, m)
    for layout in ("aligned", "odd"):
        got = shortwave(engine, inputs, layout, whole(inputs), from_last, knots=knots,
                        optics=flat)
        same(("shortwave", m, layout), got,
             shortwave(engine, inputs, layout, whole(inputs), from_last,
                       grey=inputs.grey(level)))
    inputs = sc.longwave_inputs(513, 9, 3, 11, emissivity_rows=True)
    level = level_optics(inputs)
    flat = sc.flat_optics(level, m)
    for linear in (False, True):
        for layout in ("aligned", "odd"):
            got = longwave(engine, inputs, layout, whole(inputs), from_last, linear, knots=knots,
                           optics=flat)
            same(("longwave", m, layout, linear), got,
                 longwave(engine, inputs, layout, whole(inputs), from_last, linear,
                          grey=inputs.grey(level)))


# ---------------------------------------------------------------------------------------------
# Refused calls.
def bad_tables(inputs, words):
    """[(what, knots, optics, table)]: every way a knot argument is refused."""
    knots, optics, table = inputs.knots, inputs.optics, inputs.table

    def optic(word, value):
        out = optics.copy()
        out[4, 1, word] = value
        return out

    def knot(index, value):
        out = knots.copy()
        out[index] = value
        return out

    def level(word, value):
        out = table.copy()
        out[5, word] = value
        return out
    cases_ = [("a knot that is NaN", knot(1, np.nan), optics, table),
              ("a knot that is inf", knot(2, np.inf), optics, table),
              ("knots that repeat", knot(1, knots[0]), optics, table),
              ("knots that descend", knots[::-1].copy(), optics, table),
              ("one knot", knots[:1], optics[:, :1], table),
              ("1025 knots", np.arange(1025.), np.zeros((inputs.levels, 1025, 3)), table),
              ("tau_c < 0", knots, optic(0, -1e-9), table),
              ("tau_c NaN", knots, optic(0, np.nan), table),
              ("tau_c inf", knots, optic(0, np.inf), table),
              ("omega_c > 1", knots, optic(1, 1.0000001), table),
              ("omega_c < 0", knots, optic(1, -0.1), table),
              ("omega_c NaN", knots, optic(1, np.nan), table),
              ("g_c = 1", knots, optic(2, 1.), table),
              ("g_c < 0", knots, optic(2, -0.1), table),
              ("g_c NaN", knots, optic(2, np.nan), table)]
    cases_ += [("level word %d not 0" % word, knots, optics, level(word, 0.25)) for word in words]
    return cases_


def test_bad_knot_arguments_are_refused_and_a_good_call_follows(engine):
    from pylbl_amd.engine import EngineError
    short = sc.shortwave_inputs(67, 3, 3, 1)
    long = sc.longwave_inputs(67, 3, 3, 1)
    for inputs, names, words, entry in (
            (short, SHORTWAVE_NAMES, (2, 3, 4), "lbl_path_two_stream_spectral"),
            (long, LONGWAVE_NAMES, (1, 2, 3), "lbl_path_thermal_two_stream_spectral")):
        columns, levels = inputs.columns, inputs.levels
        with Grid(engine, inputs.nu) as grid:
            def call(knots, optics, table, made, handle=grid):
                outputs = {name + "_rows": Rows(made[name]) for name in names}
                if inputs is short:
                    engine.path_two_stream_spectral(
                        Rows(made["beta"]), columns, handle, PATHS, 3, 0, table, knots, optics,
                        inputs.mu0, Rows(made["solar"]), Rows(made["work"]),
                        albedo=inputs.albedo, **outputs)
                else:
                    engine.path_thermal_two_stream_spectral(
                        Rows(made["beta"]), columns, handle, PATHS, 3, 0, table, knots, optics,
                        inputs.surface_t, Rows(made["work"]), edge_temperature=inputs.edges,
                        emissivity=inputs.emissivity, **outputs)

            def blocks():
                made = {"beta": block(inputs.beta, levels, columns, "aligned", np.nan),
                        "work": block(None, 2*levels, columns, "aligned", SENTINEL)}
                if inputs is short:
                    made["solar"] = block(inputs.solar[None, :], 1, columns, "aligned", np.nan)
                made.update(_outputs(names, inputs, "aligned"))
                return made
            made = blocks()
            ordered(engine)
            bad = bad_tables(inputs, words) + [("an unknown grid", None, None, None)]
            for what, knots, optics, table in bad:
                with pytest.raises(EngineError, match=entry):
                    if knots is None:
                        call(inputs.knots, inputs.optics, inputs.table, made, handle=grid + 1000)
                    else:
                        call(knots, optics, table, made)
                engine.synchronize()
                for name in ("work",) + tuple(names):
                    assert np.all(read(made[name]) == SENTINEL), (what, name)
            # The same engine takes the good call afterwards.
            call(inputs.knots, inputs.optics, inputs.table, made)
            engine.synchronize()
            for name in names:
                value = read(made[name], columns)
                assert np.all(np.isfinite(value)) and np.all(value != SENTINEL), name
