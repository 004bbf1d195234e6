"""lbl_path_thermal_two_stream_source fed directly (Engine.path_thermal_two_stream_source on rows
held in torch tensors) at the shapes Spectroscopy never gives it: sweep_cases' layout columns on
every layout (odd strides, bases that are not 16-byte aligned, NaN in the padding), the depths 1, 2,
3, 8, 9 and 17 (the first-face Planck alone, the carry from level to level, and every loop of
path_levels with the one row in flight of both kernels) with cloudy and clear levels alternating,
both storage orders, three paths -- random interface temperatures with inversions, jumps of 30 K
per level, one temperature throughout -- under eps = (1, 0.3, 0) and three surface temperatures
none of which is an interface's, scalar and spectral emissivity, runs of whole paths, bands, values
chosen for the branches of the layer and of the weight, and calls that must be refused.
tests/test_thermal_source_host.py proves on the CPU that the case tables of
tests/thermal_source_cases.py reach those branches.

Bounds, none taken from the code under test.  The reference is the long-double mirror of
tests/thermal_source_cases.py, continued from the float64 layer inputs.  Every flux is within
(4*E_cpu + 1e-13)*scale of it, scale = pi*max B(nu, T) over the path's interface temperatures and
T_s: E_cpu = 4.73e-15 is the worst |float64 mirror - long-double mirror|/scale that
tests/test_thermal_source_host.py measures over the same case tables (recorded as
thermal_source_cases.E_CPU = 5e-15, capped at 1e-10); the factor 4 and the floor as in
tests/test_gpu_thermal_shapes.py.  Band means are within 1e-12 * magnitude of the long-double means
of the rows the call itself wrote.  Where every temperature of a path is the same the outputs have
lbl_path_thermal_two_stream's bits.  Without scatterers every flux is within
24*2^-53*(L + 1)*scale of lbl_path_flux_source with the one angle mu = 1/D
(thermal_source_cases.PLAIN_ROUNDINGS derives the count).  The downward flux of interface 0 is 0
and the upward one has the bits of the first level's U work row.  Nothing is NaN or inf.  All
layouts of a case, and all cuts into runs of whole paths, give identical bits."""
import numpy as np
import pytest

from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_source_cases as sc
from tests.test_gpu_sweep_shapes import Grid, Rows, block, ordered, plain, read, same_bits

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
FLUX_BOUND = LD(4.*sc.E_CPU + sc.FLUX_FLOOR)
MEAN_BOUND = LD(1e-12)
NAMES = sc.NAMES
ENTRY = "lbl_path_thermal_two_stream_source"


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def run(engine, inputs, layout, runs, from_last, bands=None, wanted=NAMES, isothermal=False):
    """Every output of the entry (of lbl_path_thermal_two_stream with `isothermal`) over `runs`
    of whole paths (first level, count)."""
    n, columns, levels = inputs.levels_per_path, inputs.columns, inputs.levels
    beta = block(inputs.beta, levels, columns, layout, np.nan)
    work = block(None, 2*levels, columns, layout, SENTINEL)
    rows = {name: block(None, PATHS if name.startswith("top_") else levels, columns, layout,
                        SENTINEL) for name in wanted}
    means = {} if bands is None else {
        name: plain(PATHS if name.startswith("top_") else levels, bands.size - 1)
        for name in wanted}
    keywords = {}
    if inputs.emissivity.ndim == 2:
        keywords["emissivity_rows"] = Rows(block(inputs.emissivity, PATHS, columns, layout, np.nan))
    else:
        keywords["emissivity"] = inputs.emissivity
    with Grid(engine, inputs.nu) as grid:
        ordered(engine)
        for first, count in runs:
            part = slice(first, first + count)
            outputs = {}
            for name in wanted:
                top = name.startswith("top_")
                outputs[name + "_rows"] = Rows(rows[name] if top else rows[name][part])
                if bands is not None:
                    outputs[name + "_mean"] = Rows(means[name] if top else means[name][part])
            tables = (inputs.table[part],) if isothermal else \
                (inputs.table[part], inputs.edges[part])
            entry = engine.path_thermal_two_stream if isothermal else \
                engine.path_thermal_two_stream_source
            entry(Rows(beta[part]), columns, grid, PATHS, n, first, *tables, inputs.surface_t,
                  Rows(work[2*first:2*(first + count)]), diffusivity=inputs.diffusivity,
                  band_start=bands, from_last=from_last, **outputs, **keywords)
            engine.synchronize()
    out = {name: read(tensor, columns) for name, tensor in rows.items()}
    out.update({name + " mean": read(tensor) for name, tensor in means.items()})
    out["work"] = read(work, columns)
    assert np.array_equal(read(beta)[:, :columns], inputs.beta), "beta was written"
    return out


def check(what, inputs, got, from_last, bands=None):
    """Every flux within FLUX_BOUND*scale of the long-double mirror; finite; 0 and U at the top."""
    reference = sc.mirror(LD, inputs, from_last)
    top = reference["scale"]
    scale = {True: top, False: sc.per_level(inputs, top)}
    for name in NAMES:
        if name not in got:
            continue
        value = got[name]
        assert np.all(np.isfinite(value)), (what, name)
        error = np.abs(value.astype(LD) - reference[name])
        allowed = FLUX_BOUND*scale[name.startswith("top_")]
        lit = allowed > 0.
        worst = float(np.max(error[lit]/allowed[lit], initial=0.))
        print("%s, %s: worst error / bound %.3g" % (what, name, worst))
        assert np.all(error <= allowed), (what, name, worst)
        if bands is not None:
            expect = cases.band_means(LD, value, bands)
            mean = got[name + " mean"]
            empty = np.isnan(expect)
            assert np.array_equal(np.isnan(mean), empty) and np.count_nonzero(~empty), what
            assert np.any(empty), "no empty band"
            assert np.all(np.abs(mean[~empty].astype(LD) - expect[~empty]) <=
                          MEAN_BOUND*np.abs(expect[~empty])), (what, name, "mean")
    first = inputs.order(from_last)[:, 0]
    assert np.all(np.isfinite(got["work"])), (what, "work")
    if "top_down" in got:
        assert np.all(got["top_down"] == 0.), (what, "light from space")
    if "top_up" in got:
        assert same_bits(got["top_up"], got["work"][2*first]), (what, "U[0]")
    return reference


def whole(inputs):
    return [(0, inputs.levels)]


def per_path(inputs, reverse=False):
    n = inputs.levels_per_path
    runs = [(p*n, n) for p in range(PATHS)]
    return runs[::-1] if reverse else runs


def equal_path_has_isothermal_bits(engine, what, inputs, got, layout, from_last):
    """Path 2 of every case has one temperature at every interface and level."""
    assert np.all(inputs.interfaces[2] == sc.EQUAL_T)
    n = inputs.levels_per_path
    old = run(engine, inputs, layout, whole(inputs), from_last, isothermal=True)
    for name in NAMES:
        part = slice(2, 3) if name.startswith("top_") else slice(2*n, 3*n)
        assert same_bits(got[name][part], old[name][part]), (what, name)
    assert same_bits(got["work"][4*n:], old["work"][4*n:]), (what, "work")


@pytest.mark.parametrize("columns", cases.LAYOUT_COLUMNS)
def test_columns_on_every_layout(engine, columns):
    inputs = sc.shape_inputs(columns, 9, columns)
    base = None
    for layout in cases.LAYOUTS:
        got = run(engine, inputs, layout, whole(inputs), True)
        if base is None:
            base = got
            check((columns, layout), inputs, got, True)
        for key in base:
            assert same_bits(got[key], base[key]), (columns, layout, key)


@pytest.mark.parametrize("depth", sc.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_depths_both_orders_spectral_and_scalar_emissivity(engine, depth, from_last):
    for inputs in (sc.shape_inputs(257, depth, 40 + depth, emissivity_rows=True),
                   sc.shape_inputs(131, depth, 80 + depth)):
        base = None
        for layout, runs in (("aligned", whole(inputs)), ("odd", per_path(inputs, from_last)),
                             ("aligned", per_path(inputs, not from_last))):
            got = run(engine, inputs, layout, runs, from_last)
            if base is None:
                base = got
                check((depth, from_last, layout), inputs, got, from_last)
                equal_path_has_isothermal_bits(engine, (depth, from_last), inputs, got, layout,
                                               from_last)
            for key in base:
                assert same_bits(got[key], base[key]), (depth, from_last, layout, key)


def test_scalar_emissivity_is_its_row(engine):
    """eps = (1, 0.3, 0) under three surface temperatures, as scalars and as rows."""
    inputs = sc.shape_inputs(131, 5, 3)
    assert tuple(inputs.emissivity) == (1., 0.3, 0.) and len(set(inputs.surface_t)) == 3
    scalar = run(engine, inputs, "aligned", whole(inputs), False)
    reference = check("scalar emissivity", inputs, scalar, False)
    rows = sc.shape_inputs(131, 5, 3)
    rows.emissivity = np.repeat(inputs.emissivity[:, None], 131, axis=1)
    spectral = run(engine, rows, "offset", whole(rows), False)
    for key in scalar:
        assert same_bits(scalar[key], spectral[key]), key
    # A black surface sends up piB(T_s), not piB of the interface there; a mirror sends back what
    # comes down.
    last = inputs.order(False)[:, -1]
    lit = reference["scale"][0] > 0.
    black = tc.pi_planck(LD, inputs.nu, inputs.surface_t[0])
    assert np.all(np.abs(scalar["up"][last[0]].astype(LD) - black)[lit] <=
                  FLUX_BOUND*reference["scale"][0][lit])
    assert same_bits(scalar["up"][last[2]], scalar["down"][last[2]])


@pytest.mark.parametrize("name, columns, bands", cases.BAND_SETS)
def test_band_means(engine, name, columns, bands):
    inputs = sc.shape_inputs(columns, 3, 70)
    got = run(engine, inputs, "aligned", whole(inputs), True, bands=bands)
    check(name, inputs, got, True, bands=bands)
    cut = run(engine, inputs, "padded", per_path(inputs), True, bands=bands)
    for key in got:
        assert same_bits(cut[key], got[key]), (name, key)


@pytest.mark.parametrize("from_last", [False, True])
def test_values_chosen_for_the_branches(engine, from_last):
    """A cloud at the first level, at the last, at every level and nowhere: omega_c = 1 over beta
    = 0, beta either side of the conservative threshold, omega_c = 0.5 and 0.999999, g_c = 0 and
    0.85, tau = 3000 and 1e3, the identity layer, y = k*t across 1/2 inside a wavefront, D = 1.66
    and 2."""
    layouts = ("padded", "offset", "exact", "aligned", "odd", "aligned", "offset")
    values = sc.value_cases()
    assert len(values) == len(layouts)
    for inputs, layout in zip(values, layouts):
        runs = per_path(inputs) if layout == "padded" else whole(inputs)
        got = run(engine, inputs, layout, runs, from_last)
        check((inputs.name, inputs.diffusivity, from_last), inputs, got, from_last)
        equal_path_has_isothermal_bits(engine, inputs.name, inputs, got, layout, from_last)


@pytest.mark.parametrize("d", [1.66, 2.])
@pytest.mark.parametrize("from_last", [False, True])
def test_without_scatterers_it_is_the_linear_flux_entry_with_one_angle(engine, d, from_last):
    problem = cases.Problem(131, 9, seed=2)
    zeros = np.zeros(problem.levels)
    table = np.stack([problem.thickness, zeros, zeros, zeros, problem.temperature], axis=1)
    interfaces, table = sc.interfaces_for(table, 9, 2)
    inputs = sc.Inputs("clear", problem.nu, problem.beta, table, interfaces, tc.SURFACE_T,
                       tc.EMISSIVITY, d)
    got = run(engine, inputs, "aligned", whole(inputs), from_last)
    n, columns, levels = 9, inputs.columns, inputs.levels
    lengths = inputs.table[:, :1]/np.array([1./d])
    beta = block(inputs.beta, levels, columns, "aligned", np.nan)
    carry = block(None, PATHS, columns, "aligned", SENTINEL)
    reflection = block(None, PATHS, columns, "aligned", SENTINEL)
    sweeps = {}
    with Grid(engine, inputs.nu) as grid:
        ordered(engine)
        for up in (False, True):
            level = block(None, levels, columns, "aligned", SENTINEL)
            engine.path_flux(
                Rows(beta), columns, grid, PATHS, n, 0, lengths, np.array([1.]),
                inputs.table[:, 4], Rows(carry), Rows(reflection), Rows(level),
                surface_temperature=inputs.surface_t, surface_emissivity=inputs.emissivity,
                up=up, from_last=from_last != up, edge_temperature=inputs.edges)
            engine.synchronize()
            sweeps[up] = read(level, columns)
    at_surface = read(reflection, columns)
    order = inputs.order(from_last)
    below = np.zeros_like(sweeps[True])
    below[order[:, :-1]] = sweeps[True][order[:, 1:]]
    below[order[:, -1]] = at_surface
    expect = {"down": sweeps[False], "up": below, "top_up": sweeps[True][order[:, 0]]}
    scale = inputs.scale()
    bound = LD(sc.PLAIN_ROUNDINGS*2.**-53*(n + 1))
    for name, value in expect.items():
        size = scale if name == "top_up" else sc.per_level(inputs, scale)
        error = np.abs(got[name].astype(LD) - value.astype(LD))
        lit = size > 0.
        print("D = %g, from_last = %s, %s: worst error / bound %.3g" % (
            d, from_last, name, float(np.max(error[lit]/(bound*size[lit])))))
        assert np.all(error <= bound*size), name


def test_a_run_touches_only_its_paths_and_wanted_rows(engine):
    inputs = sc.shape_inputs(131, 5, 3)
    n = inputs.levels_per_path
    everything = run(engine, inputs, "aligned", whole(inputs), False)
    got = run(engine, inputs, "aligned", [(n, n)], False, wanted=("up", "top_down"))
    assert set(got) == {"up", "top_down", "work"}
    mine = slice(n, 2*n)
    assert same_bits(got["up"][mine], everything["up"][mine])
    assert same_bits(got["top_down"][1], everything["top_down"][1])
    assert same_bits(got["work"][2*n:4*n], everything["work"][2*n:4*n])
    for rows, kept in ((got["up"], [slice(0, n), slice(2*n, 3*n)]),
                       (got["top_down"], [slice(0, 1), slice(2, 3)]),
                       (got["work"], [slice(0, 2*n), slice(4*n, 6*n)])):
        for part in kept:
            assert np.all(rows[part] == SENTINEL)


# ---------------------------------------------------------------------------------------------
# Refused calls.
def test_rejected_calls_write_nothing_and_leave_the_engine_usable(engine):
    from pylbl_amd.engine import EngineError, PATH_CONTINUE
    inputs = sc.shape_inputs(67, 3, 1)
    columns, levels = inputs.columns, inputs.levels

    def blocks():
        made = {"beta": block(inputs.beta, levels, columns, "aligned", np.nan),
                "work": block(None, 2*levels, columns, "aligned", SENTINEL)}
        for name in NAMES:
            made[name] = block(None, PATHS if name.startswith("top_") else levels, columns,
                               "aligned", SENTINEL)
        return made

    def changed(row, column, value, of=None):
        table = (inputs.table if of is None else of).copy()
        table[row, column] = value
        return table

    cloudy = int(np.flatnonzero(inputs.cloudy)[0])
    edges = inputs.edges
    good = dict(table=inputs.table, edges=edges, ts=inputs.surface_t,
                emissivity=inputs.emissivity, emissivity_rows=False, diffusivity=1.66, first=0,
                count=levels, outputs=NAMES, alias=None, grid=0)
    bad = [dict(edges=changed(4, 0, np.nan, edges)), dict(edges=changed(4, 1, np.inf, edges)),
           dict(edges=changed(0, 0, 0., edges)), dict(edges=changed(8, 1, -5., edges)),
           # Not continuous inside a path: [r][1] != [r + 1][0] (rows 3 and 4 share path 1).
           dict(edges=changed(3, 1, edges[3, 1] + 1., edges)),
           dict(edges=changed(7, 0, edges[7, 0] - 0.5, edges)),
           dict(table=changed(4, 0, np.nan)), dict(table=changed(4, 0, -1.)),
           dict(table=changed(2, 1, np.inf)), dict(table=changed(2, 1, -0.5)),
           dict(table=changed(cloudy, 2, 1e3)),                 # w_c > tau_c
           dict(table=changed(cloudy, 3, 1.)), dict(table=changed(cloudy, 3, -0.1)),
           dict(table=changed(5, 4, 0.)), dict(table=changed(5, 4, np.nan)),
           dict(diffusivity=0.99), dict(diffusivity=2.01), dict(diffusivity=np.nan),
           dict(ts=np.array([288., 0., 300.])), dict(ts=np.array([288., np.nan, 300.])),
           dict(ts=np.array([288., np.inf, 300.])),
           dict(emissivity=None),                               # no emissivity at all
           dict(emissivity_rows=True),                          # both emissivities
           dict(emissivity=np.array([0., 1.2, 0.5])), dict(emissivity=np.array([0., -0.1, 0.5])),
           dict(first=0, count=4), dict(first=3, count=5),      # runs that cut a path
           dict(first=1, count=3),
           dict(outputs=()), dict(alias="beta"), dict(alias="work"), dict(grid=1000)]
    # A jump between two paths is no discontinuity: the good table has them.
    assert edges[2, 1] != edges[3, 0] and edges[5, 1] != edges[6, 0]
    with Grid(engine, inputs.nu) as grid:
        for change in bad:
            case = dict(good, **change)
            made = blocks()
            first, count = case["first"], case["count"]
            part = slice(first, first + count)
            outputs = {name + "_rows": Rows(made[name] if name.startswith("top_")
                                            else made[name][part]) for name in case["outputs"]}
            if case["alias"] is not None:
                outputs["up_rows"] = Rows(made[case["alias"]][:count])
            ordered(engine)
            with pytest.raises(EngineError, match=ENTRY):
                engine.path_thermal_two_stream_source(
                    Rows(made["beta"][part]), columns, grid + case["grid"], PATHS, 3, first,
                    case["table"][part], case["edges"][part], case["ts"],
                    Rows(made["work"][:2*count]), diffusivity=case["diffusivity"],
                    emissivity=case["emissivity"],
                    emissivity_rows=Rows(made["up"][:PATHS]) if case["emissivity_rows"] else None,
                    **outputs)
            engine.synchronize()
            for name in ("work",) + NAMES:
                assert np.all(read(made[name]) == SENTINEL), (change, name)
        # On the C entry itself (the binding refuses some of these first): no edge table, a band
        # mean without bands, one without its rows, and a flag of the other sweeps.
        made = blocks()
        mean = plain(levels, 2)
        bands = np.array([0, 5, 67], dtype=np.int64)

        def raw(n_bands, band_start, rows, means, flags, edge=edges.ctypes.data):
            pointers = [None]*8
            for index in rows:
                pointers[index] = made["up"].data_ptr()
            for index in means:
                pointers[4 + index] = mean.data_ptr()
            return engine.lib.lbl_path_thermal_two_stream_source(
                engine.handle, made["beta"].data_ptr(), made["beta"].shape[1], columns, grid,
                PATHS, 3, 0, levels, inputs.table.ctypes.data, edge, 1.66,
                inputs.surface_t.ctypes.data, None, inputs.emissivity.ctypes.data, n_bands,
                band_start, made["work"].data_ptr(), *pointers, flags)

        ordered(engine)
        for arguments in ((0, None, [0], [0], 0), (2, bands.ctypes.data, [0], [1], 0),
                          (0, None, [0], [], PATH_CONTINUE), (0, None, [0], [], 0, None)):
            assert raw(*arguments) != 0, arguments
            assert ENTRY.encode() in engine.lib.lbl_last_error(engine.handle)
        engine.synchronize()
        for name in ("work",) + NAMES:
            assert np.all(read(made[name]) == SENTINEL), name
        assert np.all(read(mean) == SENTINEL)
        # The same call without the fault is taken: the engine is usable.
        assert raw(2, bands.ctypes.data, [0], [0], 0) == 0
        engine.synchronize()
        assert np.all(np.isfinite(read(mean))) and np.all(read(made["up"], columns) != SENTINEL)
