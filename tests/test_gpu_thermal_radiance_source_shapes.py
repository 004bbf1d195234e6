"""lbl_path_thermal_radiance_source fed directly (Engine.path_thermal_radiance_source on rows held
in torch tensors), with flux rows made by the numpy mirror of the linear-in-tau flux entry so that
the kernel is tested alone, at the shapes Spectroscopy never gives it: thermal_cases.shape_cases'
problems -- sweep_cases' layout columns on every layout (odd strides, bases that are not 16-byte
aligned, NaN in the padding: vector and scalar rows, partial wavefronts), the depths 1, 2, 3, 8, 9,
16 and 17 with cloudy and clear levels alternating, both storage orders, scalar and spectral
emissivity, the band sets -- with thermal_source_cases' interface temperatures (inversions, 30 K
jumps per level, one temperature throughout, T_s apart from the surface interface), viewed along
mu = (1, 0.6, 0.05); runs of one path and of several; the values chosen for the branches of the
level (clear, conservative, general with y > 0, y < 0 and y = 0, k*t = 1000 and 1700, y = k*t across
1/2) and calls that must be refused.

Bounds, none taken from the code under test.  The reference is the long-double mirror of
tests/thermal_radiance_source_cases.py, continued from the float64 layer inputs and fed the same
float64 flux rows.  Every radiance is within (4*E_cpu + 1e-13)*scale of it, scale = max B(nu, T)
over the path's interface temperatures and T_s: E_cpu = 8.78e-10 is the worst |float64 mirror -
long-double mirror|/scale that tests/test_thermal_radiance_source_host.py measures over the same
case tables (recorded as thermal_radiance_source_cases.E_CPU = 9e-10); the factor 4 because the
device's exp and expm1 are a few ulp where numpy's are about one.  The brightness temperature is
within 1e-13*T of the long-double inversion of the radiance the call itself wrote.  Band means are
within 1e-12 * magnitude of the long-double means of the rows the call itself wrote.  Nothing is NaN
or inf.  All layouts of a case, and all cuts into runs of whole paths, give identical bits; beta
and the flux rows are unwritten."""
import numpy as np
import pytest

from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_source_cases as vc
from tests.test_gpu_sweep_shapes import Grid, Rows, block, ordered, plain, read, same_bits

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
BOUND = LD(4.*vc.E_CPU + vc.FLOOR)
BRIGHTNESS_BOUND = LD(1e-13)
MEAN_BOUND = LD(1e-12)
NAMES = ("radiance", "brightness")
MU = np.array(vc.MU)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


@pytest.fixture(scope="module")
def shapes():
    """thermal_cases.shape_cases' problems with their interfaces, formed once: {(columns, depth,
    rows): [(inputs, mu, from_last), ...]}."""
    table = {}
    for inputs, mu, from_last in vc.shape_cases():
        key = (inputs.columns, inputs.levels_per_path, inputs.emissivity.ndim == 2)
        table.setdefault(key, []).append((inputs, mu, from_last))
    return table


def run(engine, inputs, mu, layout, runs, from_last, bands=None, wanted=NAMES, fluxes=None):
    """Every output of the entry over `runs` of whole paths (first level, count)."""
    n, columns, levels = inputs.levels_per_path, inputs.columns, inputs.levels
    fluxes = reference(inputs, mu, from_last)[0] if fluxes is None else fluxes
    beta = block(inputs.beta, levels, columns, layout, np.nan)
    up = block(fluxes["up"], levels, columns, layout, np.nan)
    down = block(fluxes["down"], levels, columns, layout, np.nan)
    rows = {name: block(None, PATHS, columns, layout, SENTINEL) for name in wanted}
    mean = None if bands is None else plain(PATHS, bands.size - 1)
    edges = inputs.edges.copy()
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
            engine.path_thermal_radiance_source(
                Rows(beta[part]), columns, grid, PATHS, n, first, inputs.table[part], edges[part],
                mu, inputs.surface_t, Rows(up[part]), Rows(down[part]),
                diffusivity=inputs.diffusivity, band_start=bands, from_last=from_last, **outputs,
                **keywords)
            engine.synchronize()
    out = {name: read(tensor, columns) for name, tensor in rows.items()}
    if mean is not None:
        out["radiance mean"] = read(mean)
    assert np.array_equal(read(beta)[:, :columns], inputs.beta), "beta was written"
    assert same_bits(read(up)[:, :columns], fluxes["up"]), "up_rows were written"
    assert same_bits(read(down)[:, :columns], fluxes["down"]), "down_rows were written"
    assert same_bits(edges, inputs.edges), "the edge table was written"
    return out


def reference(inputs, mu, from_last):
    """The flux rows and the long-double mirror of a problem, formed once."""
    store = inputs.__dict__.setdefault("_view", {})
    key = (tuple(mu), from_last)
    if key not in store:
        fluxes = vc.flux_rows(inputs, from_last)
        store[key] = (fluxes, vc.mirror(LD, inputs, mu, from_last, fluxes))
    return store[key]


def check(what, inputs, mu, got, from_last, bands=None):
    """Every radiance within BOUND*scale of the long-double mirror; finite; the brightness
    temperature the inversion of the radiance."""
    _, expect = reference(inputs, mu, from_last)
    scale = expect["scale"]
    value = got["radiance"]
    assert np.all(np.isfinite(value)), what
    error = np.abs(value.astype(LD) - expect["radiance"])
    allowed = BOUND*scale
    lit = allowed > 0.
    worst = float(np.max(error[lit]/allowed[lit], initial=0.))
    print("%s: worst error / bound %.3g" % (what, worst))
    assert np.all(error <= allowed), (what, worst)
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


@pytest.mark.parametrize("columns", cases.LAYOUT_COLUMNS)
def test_columns_on_every_layout(engine, shapes, columns):
    (inputs, mu, from_last), = [case for case in shapes[(columns, 9, False)] if case[2]][:1]
    base = None
    for layout in cases.LAYOUTS:
        got = run(engine, inputs, mu, layout, whole(inputs), from_last)
        if base is None:
            base = got
            check((columns, layout), inputs, mu, got, from_last)
        for key in base:
            assert same_bits(got[key], base[key]), (columns, layout, key)


@pytest.mark.parametrize("depth", tc.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_depths_both_orders_and_spectral_emissivity(engine, shapes, depth, from_last):
    (inputs, mu, _), = [case for case in shapes[(513, depth, True)] if case[2] == from_last]
    base = None
    # One run, runs of one path in both orders, and a run of two paths behind a run of one.
    n = inputs.levels_per_path
    for layout, runs in (("aligned", whole(inputs)), ("odd", per_path(inputs, from_last)),
                         ("aligned", per_path(inputs, not from_last)),
                         ("offset", [(n, 2*n), (0, n)])):
        got = run(engine, inputs, mu, layout, runs, from_last)
        if base is None:
            base = got
            check((depth, from_last, layout), inputs, mu, got, from_last)
        for key in base:
            assert same_bits(got[key], base[key]), (depth, from_last, layout, key)


def test_scalar_emissivity_is_its_row(engine):
    """eps = (1, 0.3, 0) under three surface temperatures, as scalars and as rows."""
    inputs = vc.shape_inputs(131, 5, 3)
    assert tuple(inputs.emissivity) == (1., 0.3, 0.) and len(set(inputs.surface_t)) == 3
    scalar = run(engine, inputs, MU, "aligned", whole(inputs), False)
    check("scalar emissivity", inputs, MU, scalar, False)
    rows = vc.shape_inputs(131, 5, 3)
    rows.emissivity = np.repeat(inputs.emissivity[:, None], 131, axis=1)
    spectral = run(engine, rows, MU, "offset", whole(rows), False)
    for key in scalar:
        assert same_bits(scalar[key], spectral[key]), key


@pytest.mark.parametrize("name, columns, bands", cases.BAND_SETS)
def test_band_means(engine, shapes, name, columns, bands):
    inputs, mu, from_last = shapes[(columns, 3, False)][0]
    got = run(engine, inputs, mu, "aligned", whole(inputs), from_last, bands=bands,
              wanted=("radiance",))
    check(name, inputs, mu, got, from_last, bands=bands)
    cut = run(engine, inputs, mu, "padded", per_path(inputs), from_last, bands=bands,
              wanted=("radiance",))
    for key in got:
        assert same_bits(cut[key], got[key]), (name, key)


@pytest.mark.parametrize("from_last", [False, True])
def test_values_chosen_for_the_branches(engine, from_last):
    """Clouds at the first level, at the last, at every level and nowhere (the clear, the
    conservative and the general branch, beta either side of the conservative threshold, tau =
    3000, the identity layer, D = 1.66, 2 and 1), y = k*t across 1/2, k*mu = 1 exactly and 1 +-
    1e-9, and k*t = 1000 and 1700 under a small t/mu, each with inversions, 30 K jumps and one
    temperature throughout."""
    layouts = ("padded", "offset", "exact", "aligned", "odd", "aligned", "odd", "padded", "exact",
               "offset")
    value_cases = vc.value_cases()
    assert len(value_cases) == len(layouts)
    for (inputs, mu), layout in zip(value_cases, layouts):
        runs = per_path(inputs) if layout == "padded" else whole(inputs)
        got = run(engine, inputs, mu, layout, runs, from_last)
        check((inputs.name, inputs.diffusivity, from_last), inputs, mu, got, from_last)


def test_without_scatterers_it_has_the_bits_of_path_radiance_source(engine):
    """No scatterers, eps = 1 and mu = 1: lbl_path_radiance_source's result from B(T_s), bit for
    bit."""
    from tests import linear_source_cases as ls
    from tests import thermal_cases as tc
    from tests import thermal_source_cases as sc
    problem = cases.Problem(513, 9, seed=2)
    zeros = np.zeros(problem.levels)
    table = np.stack([problem.thickness, zeros, zeros, zeros, problem.temperature], axis=1)
    inputs = sc.Inputs("clear", problem.nu, problem.beta, table, ls.interfaces_for(problem, 2),
                       tc.SURFACE_T, np.ones(3))
    for from_last in (False, True):
        got = run(engine, inputs, np.ones(3), "aligned", whole(inputs), from_last)
        check(("clear", from_last), inputs, np.ones(3), got, from_last)
        beta = block(inputs.beta, inputs.levels, 513, "aligned", np.nan)
        carry = block(None, PATHS, 513, "aligned", SENTINEL)
        radiance = block(None, PATHS, 513, "aligned", SENTINEL)
        brightness = block(None, PATHS, 513, "aligned", SENTINEL)
        with Grid(engine, inputs.nu) as grid:
            ordered(engine)
            engine.path_radiance(Rows(beta), 513, grid, PATHS, 9, 0, problem.thickness,
                                 problem.temperature, Rows(carry),
                                 boundary_temperature=inputs.surface_t,
                                 boundary_emissivity=np.ones(3), radiance=Rows(radiance),
                                 brightness_temperature=Rows(brightness),
                                 from_last=not from_last, edge_temperature=inputs.edges)
            engine.synchronize()
        assert same_bits(got["radiance"], read(radiance, 513))
        assert same_bits(got["brightness"], read(brightness, 513))


def test_one_temperature_on_cloudy_paths_has_the_bits_of_the_isothermal_entry(engine):
    """Path 2 of the pole table: every level cloudy, every interface and level at one temperature.
    Fed the isothermal entry's own flux rows (which the linear flux entry reproduces there bit for
    bit) the entry returns lbl_path_thermal_radiance's bits on that path."""
    from tests import thermal_radiance_cases as rc
    inputs = vc.pole()
    n = inputs.levels_per_path
    for from_last in (False, True):
        fluxes = rc.flux_rows(inputs.isothermal(), from_last)
        got = run(engine, inputs, inputs.mu, "aligned", [(2*n, n)], from_last, fluxes=fluxes)
        beta = block(inputs.beta, inputs.levels, inputs.columns, "aligned", np.nan)
        up = block(fluxes["up"], inputs.levels, inputs.columns, "aligned", np.nan)
        down = block(fluxes["down"], inputs.levels, inputs.columns, "aligned", np.nan)
        rows = {name: block(None, PATHS, inputs.columns, "aligned", SENTINEL) for name in NAMES}
        part = slice(2*n, 3*n)
        with Grid(engine, inputs.nu) as grid:
            ordered(engine)
            engine.path_thermal_radiance(
                Rows(beta[part]), inputs.columns, grid, PATHS, n, 2*n, inputs.table[part],
                inputs.mu, inputs.surface_t, Rows(up[part]), Rows(down[part]),
                diffusivity=inputs.diffusivity, emissivity=inputs.emissivity, from_last=from_last,
                **{name + "_rows": Rows(rows[name]) for name in NAMES})
            engine.synchronize()
        for name in NAMES:
            assert same_bits(got[name][2], read(rows[name], inputs.columns)[2]), (name, from_last)
            assert np.all(got[name][:2] == SENTINEL)


def test_a_run_touches_only_its_paths_and_wanted_rows(engine):
    inputs = vc.shape_inputs(131, 5, 3)
    n = inputs.levels_per_path
    everything = run(engine, inputs, MU, "aligned", whole(inputs), False)
    got = run(engine, inputs, MU, "aligned", [(n, n)], False, wanted=("brightness",))
    assert set(got) == {"brightness"}
    assert same_bits(got["brightness"][1], everything["brightness"][1])
    assert np.all(got["brightness"][[0, 2]] == SENTINEL)


# ---------------------------------------------------------------------------------------------
# Refused calls.
def test_rejected_calls_write_nothing_and_leave_the_engine_usable(engine):
    from pylbl_amd.engine import EngineError, PATH_CONTINUE
    inputs = vc.shape_inputs(67, 3, 1)
    columns, levels = inputs.columns, inputs.levels
    fluxes = vc.flux_rows(inputs, False)

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
                count=levels, outputs=NAMES, alias=None, grid=0, mu=MU)
    bad = [dict(edges=edged(4, 0, np.nan)), dict(edges=edged(4, 1, np.inf)),
           dict(edges=edged(0, 0, 0.)), dict(edges=edged(8, 1, -250.)),
           # Not continuous within a path: one side of an inner interface moved.
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
           dict(grid=1000)]
    # The two sides of the interface between two paths may differ: the table is continuous
    # within a path only.
    assert inputs.edges[2, 1] != inputs.edges[3, 0]
    with Grid(engine, inputs.nu) as grid:
        for change in bad:
            case = dict(good, **change)
            made = blocks()
            first, count = case["first"], case["count"]
            part = slice(first, first + count)
            outputs = {name + "_rows": Rows(made[name][:PATHS]) for name in case["outputs"]}
            if case["alias"] is not None:
                outputs["radiance_rows"] = Rows(made[case["alias"]][part])
            ordered(engine)
            with pytest.raises(EngineError, match="lbl_path_thermal_radiance_source"):
                engine.path_thermal_radiance_source(
                    Rows(made["beta"][part]), columns, grid + case["grid"], PATHS, 3, first,
                    case["table"][part], case["edges"][part], case["mu"], case["ts"],
                    Rows(made["up"][part]), Rows(made["down"][part]),
                    diffusivity=case["diffusivity"], emissivity=case["emissivity"],
                    emissivity_rows=Rows(made["spare"][:PATHS]) if case["emissivity_rows"]
                    else None, **outputs)
            engine.synchronize()
            untouched(made, change)
        # On the C entry itself (the binding refuses some of these first): a null edge table, a
        # missing flux row, a band mean without bands, one without its rows, and a flag of the
        # other sweeps.
        made = blocks()
        mean = plain(PATHS, 2)
        bands = np.array([0, 5, 67], dtype=np.int64)

        def raw(n_bands, band_start, edges, up, down, radiance, brightness, means, flags):
            pointer = lambda name: made[name].data_ptr() if name else None      # noqa: E731
            return engine.lib.lbl_path_thermal_radiance_source(
                engine.handle, made["beta"].data_ptr(), made["beta"].shape[1], columns, grid,
                PATHS, 3, 0, levels, inputs.table.ctypes.data,
                inputs.edges.ctypes.data if edges else None, 1.66, MU.ctypes.data,
                inputs.surface_t.ctypes.data, None, inputs.emissivity.ctypes.data, pointer(up),
                pointer(down), n_bands, band_start, pointer(radiance), pointer(brightness),
                mean.data_ptr() if means else None, flags)

        ordered(engine)
        for arguments in ((0, None, False, "up", "down", "radiance", None, False, 0),
                          (0, None, True, None, "down", "radiance", None, False, 0),
                          (0, None, True, "up", None, "radiance", None, False, 0),
                          (0, None, True, "up", "down", "radiance", None, True, 0),
                          (2, bands.ctypes.data, True, "up", "down", None, "brightness", True, 0),
                          (0, None, True, "up", "down", "radiance", None, False, PATH_CONTINUE)):
            assert raw(*arguments) != 0, arguments
            assert b"lbl_path_thermal_radiance_source" in engine.lib.lbl_last_error(engine.handle)
        engine.synchronize()
        untouched(made, "raw")
        assert np.all(read(mean) == SENTINEL)
        # The same call without the fault is taken: the engine is usable.
        assert raw(2, bands.ctypes.data, True, "up", "down", "radiance", None, True, 0) == 0
        engine.synchronize()
        assert np.all(np.isfinite(read(mean)))
        assert np.all(read(made["radiance"], columns)[:PATHS] != SENTINEL)
        assert np.all(read(made["radiance"])[PATHS:] == SENTINEL)
