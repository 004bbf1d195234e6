"""lbl_path_thermal_radiance_observer fed directly (Engine.path_thermal_radiance_observer on rows
held in torch tensors), with flux rows made by the numpy mirrors of the two flux entries so that
the kernel is tested alone, at the shapes of tests/test_gpu_thermal_radiance_shapes.py:
thermal_cases.shape_cases' problems -- sweep_cases' layout columns on every layout (vector and
scalar rows, partial wavefronts, NaN in the padding), the depths 1, 2, 3, 8, 9, 16 and 17 with
cloudy and clear levels alternating, both storage orders, scalar and spectral emissivity, the band
sets --, isothermal and with thermal_source_cases' interface temperatures, viewed along mu = (1,
0.6, 0.05), with the observer at every interface (depths <= 3) or at {0, 1, L//2, L - 1, L}
levels from the start of the view, looking down and up, and in every call once with different n_p
across the three paths; runs of one path and of several; the smallest case that an observer made
by cutting the step count of the existing view sweep would get wrong; n_p = L looking down against
the rows of the two existing entries, bit for bit, on the value cases; and calls that must be
refused.

Bounds, none taken from the code under test.  The reference is the long-double mirror of
tests/thermal_radiance_observer_cases.py, continued from the float64 layer inputs and fed the same
float64 flux rows.  Every radiance is within (4*E_cpu + 1e-13)*scale of it, scale = max B(nu, T)
over the path's temperatures and T_s; E_cpu is the worst |float64 mirror - long-double mirror|/scale
that tests/test_thermal_radiance_observer_host.py measures over the case tables, observers and
directions of the problem's source (2.11e-11 isothermal, 2.02e-9 linear in tau; recorded as
thermal_radiance_observer_cases.E_CPU and E_CPU_LINEAR); the factor 4 because the device's exp and
expm1 are a few ulp where numpy's are about one.  The brightness temperature is within 1e-13*T of
the long-double inversion of the radiance the call itself wrote, and 0 where that radiance is 0.
Band means are within 1e-12 * magnitude of the long-double means of the rows the call itself wrote.
Nothing is NaN or inf.  All layouts of a case, and all cuts into runs of whole paths, give
identical bits; beta and the flux rows are unwritten."""
import numpy as np
import pytest

from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_radiance_observer_cases as oc
from tests import thermal_radiance_source_cases as src
from tests.test_gpu_sweep_shapes import Grid, Rows, block, ordered, plain, read, same_bits

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
BRIGHTNESS_BOUND = LD(1e-13)
MEAN_BOUND = LD(1e-12)
NAMES = ("radiance", "brightness")
MU = np.array(oc.MU)
SOURCES = ("isothermal", "linear")


def bound(inputs):
    return LD(4.*(oc.E_CPU_LINEAR if oc.linear(inputs) else oc.E_CPU) + oc.FLOOR)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


@pytest.fixture(scope="module")
def shapes():
    """thermal_cases.shape_cases' problems of both sources, formed once: {(source, columns, depth,
    rows): [(inputs, mu, from_last), ...]}."""
    table = {}
    for source, module in zip(SOURCES, (rc, src)):
        for inputs, mu, from_last in module.shape_cases():
            key = (source, inputs.columns, inputs.levels_per_path, inputs.emissivity.ndim == 2)
            table.setdefault(key, []).append((inputs, mu, from_last))
    return table


def run(engine, inputs, mu, layout, runs, from_last, passed, up, bands=None, wanted=NAMES,
        fluxes=None):
    """Every output of the entry over `runs` of whole paths (first level, count); fluxes: the
    flux rows it reads (None: the float64 mirror's)."""
    n, columns, levels = inputs.levels_per_path, inputs.columns, inputs.levels
    fluxes = flux_rows(inputs, from_last) if fluxes is None else fluxes
    beta = block(inputs.beta, levels, columns, layout, np.nan)
    rows_up = block(fluxes["up"], levels, columns, layout, np.nan)
    rows_down = block(fluxes["down"], levels, columns, layout, np.nan)
    rows = {name: block(None, PATHS, columns, layout, SENTINEL) for name in wanted}
    mean = None if bands is None else plain(PATHS, bands.size - 1)
    edges = inputs.edges.copy() if oc.linear(inputs) else None
    passed = np.array(passed, dtype=np.int32)
    keywords = {}
    if inputs.emissivity.ndim == 2:
        keywords["emissivity_rows"] = Rows(block(inputs.emissivity, PATHS, columns, layout, np.nan))
    else:
        keywords["emissivity"] = inputs.emissivity
    with Grid(engine, inputs.nu) as grid:
        ordered(engine)
        for first, count in runs:
            part = slice(first, first + count)
            outputs = {name + "_rows": Rows(rows[name]) for name in wanted}
            if bands is not None:
                outputs["radiance_mean"] = Rows(mean)
            engine.path_thermal_radiance_observer(
                Rows(beta[part]), columns, grid, PATHS, n, first, inputs.table[part], mu, passed,
                inputs.surface_t, Rows(rows_up[part]), Rows(rows_down[part]),
                edge_temperature=None if edges is None else edges[part], view_up=up,
                diffusivity=inputs.diffusivity, band_start=bands, from_last=from_last, **outputs,
                **keywords)
            engine.synchronize()
    out = {name: read(tensor, columns) for name, tensor in rows.items()}
    if mean is not None:
        out["radiance mean"] = read(mean)
    assert np.array_equal(read(beta)[:, :columns], inputs.beta), "beta was written"
    assert same_bits(read(rows_up)[:, :columns], fluxes["up"]), "up_rows were written"
    assert same_bits(read(rows_down)[:, :columns], fluxes["down"]), "down_rows were written"
    if edges is not None:
        assert same_bits(edges, inputs.edges), "the edge table was written"
    return out


def flux_rows(inputs, from_last):
    """The float64 flux rows of a problem, formed once."""
    store = inputs.__dict__.setdefault("_observer_fluxes", {})
    if from_last not in store:
        store[from_last] = oc.flux_rows(inputs, from_last)
    return store[from_last]


def reference(inputs, mu, from_last, passed, up):
    """The long-double mirror of a view, formed once."""
    store = inputs.__dict__.setdefault("_observer_view", {})
    key = (tuple(mu), from_last, tuple(int(n) for n in passed), bool(up))
    if key not in store:
        store[key] = oc.mirror(LD, inputs, mu, from_last, passed, up, flux_rows(inputs, from_last))
    return store[key]


def check(what, inputs, mu, got, from_last, passed, up, bands=None):
    """Every radiance within bound*scale of the long-double mirror; finite; the brightness
    temperature the inversion of the radiance."""
    expect = reference(inputs, mu, from_last, passed, up)
    scale = expect["scale"]
    value = got["radiance"]
    assert np.all(np.isfinite(value)), what
    error = np.abs(value.astype(LD) - expect["radiance"])
    allowed = bound(inputs)*scale
    lit = allowed > 0.
    worst = float(np.max(error[lit]/allowed[lit], initial=0.))
    print("%s n_p=%s up=%s: worst error / bound %.3g" % (what, list(passed), up, worst))
    assert np.all(error <= allowed), (what, list(passed), up, worst)
    # A path whose ray passes no level holds its start value: 0 looking up.
    still = np.asarray(passed) == 0
    if up and np.any(still):
        assert np.all(value[still] == 0.), what
    if "brightness" in got:
        assert np.all(np.isfinite(got["brightness"])), what
        inverted = cases.brightness(LD, inputs.nu[None, :], value)
        assert np.all(np.abs(got["brightness"].astype(LD) - inverted) <=
                      BRIGHTNESS_BOUND*inverted), (what, "brightness")
        assert np.array_equal(got["brightness"] == 0., inverted == 0.)
    if bands is not None:
        means = cases.band_means(LD, value, bands)
        mean = got["radiance mean"]
        empty = np.isnan(means)
        assert np.array_equal(np.isnan(mean), empty) and np.count_nonzero(~empty), what
        assert np.any(empty), "no empty band"
        assert np.all(np.abs(mean[~empty].astype(LD) - means[~empty]) <=
                      MEAN_BOUND*np.abs(means[~empty])), (what, "mean")
    return expect


def whole(inputs):
    return [(0, inputs.levels)]


def per_path(inputs, reverse=False):
    n = inputs.levels_per_path
    runs = [(p*n, n) for p in range(PATHS)]
    return runs[::-1] if reverse else runs


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("columns", cases.LAYOUT_COLUMNS)
def test_columns_on_every_layout(engine, shapes, columns, source):
    """Every observer on vector rows; the call with three different n_p on every layout."""
    (inputs, mu, from_last), = [case for case in shapes[(source, columns, 9, False)]
                                if case[2]][:1]
    calls = oc.observers(9)
    for up in (False, True):
        for passed in calls[:-1]:
            got = run(engine, inputs, mu, "aligned", whole(inputs), from_last, passed, up)
            check((source, columns), inputs, mu, got, from_last, passed, up)
        base = None
        for layout in cases.LAYOUTS:
            got = run(engine, inputs, mu, layout, whole(inputs), from_last, calls[-1], up)
            if base is None:
                base = got
                check((source, columns, layout), inputs, mu, got, from_last, calls[-1], up)
            for key in base:
                assert same_bits(got[key], base[key]), (columns, layout, key, up)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("depth", tc.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_depths_both_orders_and_spectral_emissivity(engine, shapes, depth, from_last, source):
    (inputs, mu, _), = [case for case in shapes[(source, 513, depth, True)]
                        if case[2] == from_last]
    n = inputs.levels_per_path
    calls = oc.observers(depth)
    for up in (False, True):
        for passed in calls[:-1]:
            got = run(engine, inputs, mu, "odd", whole(inputs), from_last, passed, up)
            check((source, depth, from_last), inputs, mu, got, from_last, passed, up)
        # The call with different n_p: one run, runs of one path in both orders, and a run of
        # two paths behind a run of one.
        base = None
        for layout, runs in (("aligned", whole(inputs)), ("odd", per_path(inputs, from_last)),
                             ("aligned", per_path(inputs, not from_last)),
                             ("offset", [(n, 2*n), (0, n)])):
            got = run(engine, inputs, mu, layout, runs, from_last, calls[-1], up)
            if base is None:
                base = got
                check((source, depth, from_last, layout), inputs, mu, got, from_last, calls[-1],
                      up)
            for key in base:
                assert same_bits(got[key], base[key]), (depth, from_last, layout, key, up)


def test_an_observer_under_clear_sky_reads_the_down_row_above_the_cloud(engine):
    """2 levels, a cloud in the level nearer the surface, the observer between the levels, looking
    down: the cloud's F_against is the down row at interface 1, not the 0 of the path's space
    end that a sweep with its step count cut would take there."""
    inputs = oc.pitfall()
    passed = np.full(PATHS, 1)
    for layout in ("aligned", "odd"):
        got = run(engine, inputs, MU, layout, whole(inputs), False, passed, False)
        check("pitfall", inputs, MU, got, False, passed, False)
    # What the cut sweep would give lies far outside the bound.
    fluxes = flux_rows(inputs, False)
    wrong = dict(fluxes, down=fluxes["down"].copy())
    wrong["down"][inputs.order(False)[:, 0]] = 0.
    bad = oc.mirror(LD, inputs, MU, False, passed, False, wrong)
    expect = reference(inputs, MU, False, passed, False)
    assert np.max(np.abs(bad["radiance"] - expect["radiance"])/expect["scale"]) > \
        1e6*bound(inputs)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name, columns, bands", cases.BAND_SETS)
def test_band_means(engine, shapes, name, columns, bands, source):
    inputs, mu, from_last = shapes[(source, columns, 3, False)][0]
    passed = oc.observers(3)[-1]
    for up in (False, True):
        got = run(engine, inputs, mu, "aligned", whole(inputs), from_last, passed, up,
                  bands=bands, wanted=("radiance",))
        check(name, inputs, mu, got, from_last, passed, up, bands=bands)
        cut = run(engine, inputs, mu, "padded", per_path(inputs), from_last, passed, up,
                  bands=bands, wanted=("radiance",))
        for key in got:
            assert same_bits(cut[key], got[key]), (name, key, up)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("from_last", [False, True])
def test_the_whole_view_down_has_the_bits_of_the_existing_entries(engine, from_last, source):
    """n_p = L looking down on the value cases (the clear, the conservative and the general
    branch, tau = 3000, the identity layer, k*mu = 1 exactly and 1 +- 1e-9, k*t = 1000 and 1700):
    the rows of lbl_path_thermal_radiance and lbl_path_thermal_radiance_source, bit for bit."""
    module = src if source == "linear" else rc
    for inputs, mu in module.value_cases():
        n, columns, levels = inputs.levels_per_path, inputs.columns, inputs.levels
        passed = np.full(PATHS, n)
        got = run(engine, inputs, mu, "aligned", whole(inputs), from_last, passed, False)
        check((inputs.name, inputs.diffusivity), inputs, mu, got, from_last, passed, False)
        fluxes = flux_rows(inputs, from_last)
        beta = block(inputs.beta, levels, columns, "aligned", np.nan)
        up = block(fluxes["up"], levels, columns, "aligned", np.nan)
        down = block(fluxes["down"], levels, columns, "aligned", np.nan)
        rows = {name: block(None, PATHS, columns, "aligned", SENTINEL) for name in NAMES}
        outputs = {name + "_rows": Rows(rows[name]) for name in NAMES}
        common = dict(diffusivity=inputs.diffusivity, emissivity=inputs.emissivity,
                      from_last=from_last)
        with Grid(engine, inputs.nu) as grid:
            ordered(engine)
            if source == "linear":
                engine.path_thermal_radiance_source(
                    Rows(beta), columns, grid, PATHS, n, 0, inputs.table, inputs.edges, mu,
                    inputs.surface_t, Rows(up), Rows(down), **common, **outputs)
            else:
                engine.path_thermal_radiance(
                    Rows(beta), columns, grid, PATHS, n, 0, inputs.table, mu, inputs.surface_t,
                    Rows(up), Rows(down), **common, **outputs)
            engine.synchronize()
        for name in NAMES:
            assert same_bits(got[name], read(rows[name], columns)), (inputs.name, name)
        # The view up through the same values stays within its bound.
        got = run(engine, inputs, mu, "odd", whole(inputs), from_last, passed, True)
        check((inputs.name, inputs.diffusivity), inputs, mu, got, from_last, passed, True)


@pytest.mark.parametrize("source", SOURCES)
def test_a_run_touches_only_its_paths_and_wanted_rows(engine, source):
    inputs = (src if source == "linear" else tc).shape_inputs(131, 5, 3)
    n = inputs.levels_per_path
    passed = np.array([5, 2, 0])
    for up in (False, True):
        everything = run(engine, inputs, MU, "aligned", whole(inputs), False, passed, up)
        got = run(engine, inputs, MU, "aligned", [(n, n)], False, passed, up,
                  wanted=("brightness",))
        assert set(got) == {"brightness"}
        assert same_bits(got["brightness"][1], everything["brightness"][1])
        assert np.all(got["brightness"][[0, 2]] == SENTINEL)
        # Path 2 passes no level: its row is written all the same.
        assert np.all(everything["radiance"][2] != SENTINEL)


# ---------------------------------------------------------------------------------------------
# Refused calls.
def test_rejected_calls_write_nothing_and_leave_the_engine_usable(engine):
    from pylbl_amd.engine import EngineError, PATH_CONTINUE
    inputs = src.shape_inputs(67, 3, 1)
    columns, levels = inputs.columns, inputs.levels
    fluxes = oc.flux_rows(inputs, False)

    def blocks():
        made = {"beta": block(inputs.beta, levels, columns, "aligned", np.nan),
                "up": block(fluxes["up"], levels, columns, "aligned", np.nan),
                "down": block(fluxes["down"], levels, columns, "aligned", np.nan)}
        for name in NAMES + ("spare",):
            made[name] = block(None, levels, columns, "aligned", SENTINEL)
        return made

    def changed(row, column, value):
        table = inputs.table.copy()
        table[row, column] = value
        return table

    def edged(row, side, value):
        edges = inputs.edges.copy()
        edges[row, side] = value
        return edges

    def untouched(made, change):
        for name in NAMES + ("spare",):
            assert np.all(read(made[name]) == SENTINEL), (change, name)
        assert np.array_equal(read(made["beta"])[:, :columns], inputs.beta), change
        assert same_bits(read(made["up"])[:, :columns], fluxes["up"]), change
        assert same_bits(read(made["down"])[:, :columns], fluxes["down"]), change

    cloudy = int(np.flatnonzero(inputs.cloudy)[0])
    good = dict(table=inputs.table, edges=inputs.edges, ts=inputs.surface_t,
                emissivity=inputs.emissivity, emissivity_rows=False, diffusivity=1.66, first=0,
                count=levels, outputs=NAMES, alias=None, grid=0, mu=MU,
                passed=np.array([3, 1, 0], dtype=np.int32))
    # Every error of the entry this one extends ...
    bad = [dict(edges=edged(4, 0, np.nan)), dict(edges=edged(4, 1, np.inf)),
           dict(edges=edged(0, 0, 0.)), dict(edges=edged(8, 1, -250.)),
           dict(edges=edged(1, 0, 251.)), dict(edges=edged(7, 1, 251.)),
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
           dict(mu=np.array([1., 0., 0.5])), dict(mu=np.array([1., 1.0001, 0.5])),
           dict(mu=np.array([1., -0.5, 0.5])), dict(mu=np.array([np.nan, 1., 0.5])),
           dict(mu=np.array([1., 1., np.inf])),
           dict(first=0, count=4), dict(first=3, count=5),      # runs that cut a path
           dict(first=1, count=3),
           dict(outputs=()), dict(alias="beta"), dict(alias="up"), dict(alias="down"),
           dict(grid=1000),
           # ... and the observer's own.
           dict(passed=np.array([3, 4, 0], dtype=np.int32)),
           dict(passed=np.array([-1, 1, 0], dtype=np.int32)),
           dict(passed=np.array([0, 0, 2**31 - 1], dtype=np.int32))]
    with Grid(engine, inputs.nu) as grid:
        for up in (False, True):
            # The surface arguments are checked looking up too.
            for change in bad:
                case = dict(good, **change)
                made = blocks()
                first, count = case["first"], case["count"]
                part = slice(first, first + count)
                outputs = {name + "_rows": Rows(made[name][:PATHS]) for name in case["outputs"]}
                if case["alias"] is not None:
                    outputs["radiance_rows"] = Rows(made[case["alias"]][part])
                ordered(engine)
                with pytest.raises(EngineError, match="lbl_path_thermal_radiance_observer"):
                    engine.path_thermal_radiance_observer(
                        Rows(made["beta"][part]), columns, grid + case["grid"], PATHS, 3, first,
                        case["table"][part], case["mu"], case["passed"], case["ts"],
                        Rows(made["up"][part]), Rows(made["down"][part]),
                        edge_temperature=case["edges"][part], view_up=up,
                        diffusivity=case["diffusivity"], emissivity=case["emissivity"],
                        emissivity_rows=Rows(made["spare"][:PATHS]) if case["emissivity_rows"]
                        else None, **outputs)
                engine.synchronize()
                untouched(made, change)
        # On the C entry itself (the binding refuses some of these first): a null observer table,
        # a view_up that is neither 0 nor 1, a missing flux row, a band mean without bands, one
        # without its rows, and a flag of the other sweeps.
        made = blocks()
        mean = plain(PATHS, 2)
        bands = np.array([0, 5, 67], dtype=np.int64)
        passed = good["passed"]

        def raw(n_bands, band_start, observer, view_up, up, down, radiance, brightness, means,
                flags, edges=True):
            pointer = lambda name: made[name].data_ptr() if name else None      # noqa: E731
            return engine.lib.lbl_path_thermal_radiance_observer(
                engine.handle, made["beta"].data_ptr(), made["beta"].shape[1], columns, grid,
                PATHS, 3, 0, levels, inputs.table.ctypes.data,
                inputs.edges.ctypes.data if edges else None, 1.66, MU.ctypes.data,
                passed.ctypes.data if observer else None, view_up,
                inputs.surface_t.ctypes.data, None, inputs.emissivity.ctypes.data, pointer(up),
                pointer(down), n_bands, band_start, pointer(radiance), pointer(brightness),
                mean.data_ptr() if means else None, flags)

        ordered(engine)
        for arguments in ((0, None, False, 0, "up", "down", "radiance", None, False, 0),
                          (0, None, True, 2, "up", "down", "radiance", None, False, 0),
                          (0, None, True, -1, "up", "down", "radiance", None, False, 0),
                          (0, None, True, 1, None, "down", "radiance", None, False, 0),
                          (0, None, True, 0, "up", None, "radiance", None, False, 0),
                          (0, None, True, 1, "up", "down", "radiance", None, True, 0),
                          (2, bands.ctypes.data, True, 0, "up", "down", None, "brightness", True, 0),
                          (0, None, True, 0, "up", "down", "radiance", None, False, PATH_CONTINUE)):
            assert raw(*arguments) != 0, arguments
            assert b"lbl_path_thermal_radiance_observer" in engine.lib.lbl_last_error(engine.handle)
        engine.synchronize()
        untouched(made, "raw")
        assert np.all(read(mean) == SENTINEL)
        # The same call without the fault is taken: the engine is usable.  A null edge table is
        # no fault here: isothermal levels.
        assert raw(2, bands.ctypes.data, True, 1, "up", "down", "radiance", None, True, 0) == 0
        assert raw(0, None, True, 0, "up", "down", None, "brightness", False, 0, edges=False) == 0
        engine.synchronize()
        assert np.all(np.isfinite(read(mean)))
        assert np.all(read(made["radiance"], columns)[:PATHS] != SENTINEL)
        assert np.all(read(made["radiance"])[PATHS:] == SENTINEL)
        assert np.all(read(made["brightness"], columns)[:PATHS] != SENTINEL)
