"""lbl_path_thermal_two_stream fed directly (Engine.path_thermal_two_stream on rows held in torch
tensors) at the shapes Spectroscopy never gives it: sweep_cases' layout columns on every layout
(odd strides, bases that are not 16-byte aligned, NaN in the padding), the depths 1, A, A + 1, 2A
and 2A + 1 for the rows in flight of both kernels (A = 8 going up, 1 going down) with cloudy and
clear levels alternating, both storage orders, three paths under eps = (1, 0.3, 0) and three
surface temperatures, scalar and spectral emissivity, runs of whole paths, bands, values chosen
for the branches of the layer, and calls that must be refused.  tests/test_thermal_host.py proves
on the CPU that the case tables of tests/thermal_cases.py reach those branches.

Bounds, none taken from the code under test.  The reference is the long-double mirror of
tests/thermal_cases.py, continued from the float64 layer inputs.  Every flux is within
(4*E_cpu + 1e-13)*scale of it, scale = pi*max B(nu, T) over the path's level temperatures and T_s:
E_cpu = 6.64e-15 is the worst |float64 mirror - long-double mirror|/scale that
tests/test_thermal_host.py measures over the same case tables (recorded as thermal_cases.E_CPU =
7e-15, capped at 1e-10); the factor 4 because the device's exp and expm1 are a few ulp where
numpy's are about one and both pass through the same adding recurrences; the floor for columns
whose case happened to be benign.  The downward flux of interface 0 is 0 and the upward one has the
bits of the first level's U work row.  Band means are within 1e-12 * magnitude of the long-double
means of the rows the call itself wrote.  Nothing is NaN or inf.  All layouts of a case, and all
cuts into runs of whole paths, give identical bits."""
import numpy as np
import pytest

from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests.test_gpu_sweep_shapes import Grid, Rows, block, ordered, plain, read, same_bits

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
FLUX_BOUND = LD(4.*tc.E_CPU + tc.FLUX_FLOOR)
MEAN_BOUND = LD(1e-12)
NAMES = tc.NAMES


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def run(engine, inputs, layout, runs, from_last, bands=None, wanted=NAMES):
    """Every output of the entry over `runs` of whole paths (first level, count)."""
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
            engine.path_thermal_two_stream(
                Rows(beta[part]), columns, grid, PATHS, n, first, inputs.table[part],
                inputs.surface_t, Rows(work[2*first:2*(first + count)]),
                diffusivity=inputs.diffusivity, band_start=bands, from_last=from_last, **outputs,
                **keywords)
            engine.synchronize()
    out = {name: read(tensor, columns) for name, tensor in rows.items()}
    out.update({name + " mean": read(tensor) for name, tensor in means.items()})
    out["work"] = read(work, columns)
    assert np.array_equal(read(beta)[:, :columns], inputs.beta), "beta was written"
    return out


def check(what, inputs, got, from_last, bands=None):
    """Every flux within FLUX_BOUND*scale of the long-double mirror; finite; 0 and U at the top."""
    reference = tc.mirror(LD, inputs, from_last)
    top = reference["scale"]
    scale = {True: top, False: tc.per_level(inputs, top)}
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


@pytest.mark.parametrize("columns", cases.LAYOUT_COLUMNS)
def test_columns_on_every_layout(engine, columns):
    inputs = tc.shape_inputs(columns, 9, columns)
    base = None
    for layout in cases.LAYOUTS:
        got = run(engine, inputs, layout, whole(inputs), True)
        if base is None:
            base = got
            check((columns, layout), inputs, got, True)
        for key in base:
            assert same_bits(got[key], base[key]), (columns, layout, key)


@pytest.mark.parametrize("depth", tc.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_depths_both_orders_and_spectral_emissivity(engine, depth, from_last):
    inputs = tc.shape_inputs(513, depth, 40 + depth, emissivity_rows=True)
    base = None
    for layout, runs in (("aligned", whole(inputs)), ("odd", per_path(inputs, from_last)),
                         ("aligned", per_path(inputs, not from_last))):
        got = run(engine, inputs, layout, runs, from_last)
        if base is None:
            base = got
            check((depth, from_last, layout), inputs, got, from_last)
        for key in base:
            assert same_bits(got[key], base[key]), (depth, from_last, layout, key)


def test_scalar_emissivity_is_its_row(engine):
    """eps = (1, 0.3, 0) under three surface temperatures, as scalars and as rows."""
    inputs = tc.shape_inputs(131, 5, 3)
    assert tuple(inputs.emissivity) == (1., 0.3, 0.) and len(set(inputs.surface_t)) == 3
    scalar = run(engine, inputs, "aligned", whole(inputs), False)
    reference = check("scalar emissivity", inputs, scalar, False)
    rows = tc.shape_inputs(131, 5, 3)
    rows.emissivity = np.repeat(inputs.emissivity[:, None], 131, axis=1)
    spectral = run(engine, rows, "offset", whole(rows), False)
    for key in scalar:
        assert same_bits(scalar[key], spectral[key]), key
    # A black surface sends up piB(T_s); a mirror sends back what comes down.
    last = inputs.order(False)[:, -1]
    lit = reference["scale"][0] > 0.
    black = tc.pi_planck(LD, inputs.nu, inputs.surface_t[0])
    assert np.all(np.abs(scalar["up"][last[0]].astype(LD) - black)[lit] <=
                  FLUX_BOUND*reference["scale"][0][lit])
    assert same_bits(scalar["up"][last[2]], scalar["down"][last[2]])


@pytest.mark.parametrize("name, columns, bands", cases.BAND_SETS)
def test_band_means(engine, name, columns, bands):
    inputs = tc.shape_inputs(columns, 3, 70)
    got = run(engine, inputs, "aligned", whole(inputs), True, bands=bands)
    check(name, inputs, got, True, bands=bands)
    cut = run(engine, inputs, "padded", per_path(inputs), True, bands=bands)
    for key in got:
        assert same_bits(cut[key], got[key]), (name, key)


@pytest.mark.parametrize("from_last", [False, True])
def test_values_chosen_for_the_branches(engine, from_last):
    """A cloud at the first level, at the last and at every level: omega_c = 1 over beta = 0 (k2
    = 0 exactly), beta either side of the conservative threshold, omega_c = 0.5 and 0.999999, g_c
    = 0 and 0.85, tau = 3000 (E = 0), the identity layer (beta = 0 without tau_c), T_l from 180 to
    320 K, nu from 1 to 3000 cm-1, D = 1.66, 2 and 1."""
    for inputs, layout in zip(tc.value_cases(), ("padded", "offset", "exact", "aligned", "odd")):
        runs = per_path(inputs) if layout == "padded" else whole(inputs)
        got = run(engine, inputs, layout, runs, from_last)
        reference = check((inputs.name, inputs.diffusivity, from_last), inputs, got, from_last)
        if inputs.name == "cloud at every":
            continue
        # Under tau = 3000 in the level nearest space nothing from below gets out: the flux to
        # space is that level's own piB.
        first = inputs.order(from_last)[:, 0]
        nearest_is_clear = not inputs.cloudy[first[0]]
        if nearest_is_clear:
            thick = inputs.group == 2
            for p in range(PATHS):
                own = tc.pi_planck(LD, inputs.nu[thick], inputs.table[first[p], 4])
                assert np.all(np.abs(got["top_up"][p][thick].astype(LD) - own) <=
                              FLUX_BOUND*reference["scale"][p][thick])


def test_a_run_touches_only_its_paths_and_wanted_rows(engine):
    inputs = tc.shape_inputs(131, 5, 3)
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
    inputs = tc.shape_inputs(67, 3, 1)
    columns, levels = inputs.columns, inputs.levels

    def blocks():
        made = {"beta": block(inputs.beta, levels, columns, "aligned", np.nan),
                "work": block(None, 2*levels, columns, "aligned", SENTINEL)}
        for name in NAMES:
            made[name] = block(None, PATHS if name.startswith("top_") else levels, columns,
                               "aligned", SENTINEL)
        return made

    def changed(row, column, value):
        table = inputs.table.copy()
        table[row, column] = value
        return table

    cloudy = int(np.flatnonzero(inputs.cloudy)[0])
    good = dict(table=inputs.table, ts=inputs.surface_t, emissivity=inputs.emissivity,
                emissivity_rows=False, diffusivity=1.66, first=0, count=levels, outputs=NAMES,
                alias=None, grid=0)
    bad = [dict(table=changed(4, 0, np.nan)), dict(table=changed(4, 0, -1.)),
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
            with pytest.raises(EngineError, match="lbl_path_thermal_two_stream"):
                engine.path_thermal_two_stream(
                    Rows(made["beta"][part]), columns, grid + case["grid"], PATHS, 3, first,
                    case["table"][part], case["ts"], Rows(made["work"][:2*count]),
                    diffusivity=case["diffusivity"], emissivity=case["emissivity"],
                    emissivity_rows=Rows(made["up"][:PATHS]) if case["emissivity_rows"] else None,
                    **outputs)
            engine.synchronize()
            for name in ("work",) + NAMES:
                assert np.all(read(made[name]) == SENTINEL), (change, name)
        # On the C entry itself (the binding refuses some of these first): a band mean without
        # bands, one without its rows, and a flag of the other sweeps.
        made = blocks()
        mean = plain(levels, 2)
        bands = np.array([0, 5, 67], dtype=np.int64)

        def raw(n_bands, band_start, rows, means, flags):
            pointers = [None]*8
            for index in rows:
                pointers[index] = made["up"].data_ptr()
            for index in means:
                pointers[4 + index] = mean.data_ptr()
            return engine.lib.lbl_path_thermal_two_stream(
                engine.handle, made["beta"].data_ptr(), made["beta"].shape[1], columns, grid,
                PATHS, 3, 0, levels, inputs.table.ctypes.data, 1.66,
                inputs.surface_t.ctypes.data, None, inputs.emissivity.ctypes.data, n_bands,
                band_start, made["work"].data_ptr(), *pointers, flags)

        ordered(engine)
        for arguments in ((0, None, [0], [0], 0), (2, bands.ctypes.data, [0], [1], 0),
                          (0, None, [0], [], PATH_CONTINUE)):
            assert raw(*arguments) != 0, arguments
            assert b"lbl_path_thermal_two_stream" in engine.lib.lbl_last_error(engine.handle)
        engine.synchronize()
        for name in ("work",) + NAMES:
            assert np.all(read(made[name]) == SENTINEL), name
        assert np.all(read(mean) == SENTINEL)
        # The same call without the fault is taken: the engine is usable.
        assert raw(2, bands.ctypes.data, [0], [0], 0) == 0
        engine.synchronize()
        assert np.all(np.isfinite(read(mean))) and np.all(read(made["up"], columns) != SENTINEL)
