"""lbl_rayleigh_row and lbl_path_two_stream fed directly (Engine.rayleigh_row / path_two_stream on
rows held in torch tensors) at the shapes Spectroscopy never gives them: sweep_cases' layout columns
on every layout (odd strides, bases that are not 16-byte aligned, NaN in the padding), depths 1, 8,
9, 16 and 17 (every loop of path_levels with eight rows in flight), both storage orders, three paths under
mu0 = (1, 1e-3, 0.25) and A = (1, 0.3, 0), runs of whole paths, values chosen for the branches of
the layer, scalar and spectral albedo, bands, and calls that must be refused.
tests/test_two_stream_host.py proves on the CPU that the case tables of tests/two_stream_cases.py
reach those branches.

Bounds, none taken from the code under test.  The reference is the long-double mirror of
tests/two_stream_cases.py, continued from the float64 layer inputs.  Every flux is within
(4*E_cpu + 1e-13)*F0 of it, F0 = mu0*S the column's incident flux: E_cpu = 1.61e-11 is the worst
|float64 mirror - long-double mirror|/F0 that tests/test_two_stream_host.py measures over the same
case tables (recorded as two_stream_cases.E_CPU = 1.7e-11, capped at 1e-10); the factor 4 because
the device's exp and expm1 are a few ulp where numpy's are about one and both pass through the
same adding recurrences; the floor for columns whose case happened to be benign.  The direct
irradiance of interface 0 is F0 bit for bit.  Band means are within 1e-12 * magnitude of the
long-double means of the rows the call itself wrote.  The Rayleigh row is within (4|x| + 4)*2^-53
relative of the long-double fit, x = e*log(lambda) the exponent: one rounding each of e, the
logarithm and the product scale with |x|, exp and the last product do not.  Nothing is NaN or inf.
All layouts of a case, and all cuts into runs of whole paths, give identical bits."""
import numpy as np
import pytest

from tests import sweep_cases as cases
from tests import two_stream_cases as ts
from tests.test_gpu_sweep_shapes import Rows, block, ordered, plain, read, same_bits

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
FLUX_BOUND = LD(4.*ts.E_CPU + ts.FLUX_FLOOR)
MEAN_BOUND = LD(1e-12)
NAMES = tuple(prefix + q for prefix in ("", "top_") for q in ts.QUANTITIES)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def run(engine, inputs, layout, runs, from_last, bands=None, wanted=NAMES, sigma=True):
    """Every output of the entry over `runs` of whole paths (first level, count)."""
    n, columns, levels = inputs.levels_per_path, inputs.columns, inputs.levels
    beta = block(inputs.beta, levels, columns, layout, np.nan)
    solar = block(inputs.solar[None, :], 1, columns, layout, np.nan)
    sigma_row = block(inputs.sigma[None, :], 1, columns, layout, np.nan) if sigma else None
    work = block(None, 2*levels, columns, layout, SENTINEL)
    rows = {name: block(None, PATHS if name.startswith("top_") else levels, columns, layout,
                        SENTINEL) for name in wanted}
    means = {} if bands is None else {
        name: plain(PATHS if name.startswith("top_") else levels, bands.size - 1)
        for name in wanted}
    keywords = {}
    if inputs.albedo.ndim == 2:
        keywords["albedo_rows"] = Rows(block(inputs.albedo, PATHS, columns, layout, np.nan))
    else:
        keywords["albedo"] = inputs.albedo
    ordered(engine)
    for first, count in runs:
        part = slice(first, first + count)
        outputs = {}
        for name in wanted:
            top = name.startswith("top_")
            outputs[name + "_rows"] = Rows(rows[name] if top else rows[name][part])
            if bands is not None:
                outputs[name + "_mean"] = Rows(means[name] if top else means[name][part])
        engine.path_two_stream(
            Rows(beta[part]), columns, PATHS, n, first, inputs.table[part], inputs.mu0,
            Rows(solar), Rows(work[2*first:2*(first + count)]),
            rayleigh_row=None if sigma_row is None else Rows(sigma_row), band_start=bands,
            from_last=from_last, **outputs, **keywords)
        engine.synchronize()
    out = {name: read(tensor, columns) for name, tensor in rows.items()}
    out.update({name + " mean": read(tensor) for name, tensor in means.items()})
    out["work"] = read(work, columns)
    assert np.array_equal(read(beta)[:, :columns], inputs.beta), "beta was written"
    return out


def check(what, inputs, got, from_last, bands=None):
    """Every flux within FLUX_BOUND*F0 of the long-double mirror; finite; F0 at the top."""
    reference = ts.mirror(LD, inputs, from_last)
    f0 = reference["f0"]
    scale = {True: f0.astype(LD), False: np.repeat(f0, inputs.levels_per_path, axis=0).astype(LD)}
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
            assert np.all(np.abs(mean[~empty].astype(LD) - expect[~empty]) <=
                          MEAN_BOUND*np.abs(expect[~empty])), (what, name, "mean")
    if "top_direct" in got:
        assert same_bits(got["top_direct"], f0), (what, "F0")
    if "top_diffuse" in got:
        assert np.all(got["top_diffuse"] == 0.), (what, "diffuse light from space")
    return reference


def whole(inputs):
    return [(0, inputs.levels)]


def per_path(inputs, reverse=False):
    n = inputs.levels_per_path
    runs = [(p*n, n) for p in range(PATHS)]
    return runs[::-1] if reverse else runs


@pytest.mark.parametrize("columns", cases.LAYOUT_COLUMNS)
def test_columns_on_every_layout(engine, columns):
    inputs = ts.shape_inputs(columns, 9, columns)
    base = None
    for layout in cases.LAYOUTS:
        got = run(engine, inputs, layout, whole(inputs), True)
        if base is None:
            base = got
            check((columns, layout), inputs, got, True)
        for key in base:
            assert same_bits(got[key], base[key]), (columns, layout, key)


@pytest.mark.parametrize("depth", ts.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_depths_both_orders_and_spectral_albedo(engine, depth, from_last):
    inputs = ts.shape_inputs(513, depth, 40 + depth, albedo_rows=True)
    base = None
    for layout, runs in (("aligned", whole(inputs)), ("odd", per_path(inputs, from_last))):
        got = run(engine, inputs, layout, runs, from_last)
        if base is None:
            base = got
            check((depth, from_last, layout), inputs, got, from_last)
        for key in base:
            assert same_bits(got[key], base[key]), (depth, from_last, layout, key)


@pytest.mark.parametrize("name, columns, bands", cases.BAND_SETS)
def test_band_means(engine, name, columns, bands):
    inputs = ts.shape_inputs(columns, 3, 70)
    got = run(engine, inputs, "aligned", whole(inputs), True, bands=bands)
    check(name, inputs, got, True, bands=bands)
    cut = run(engine, inputs, "padded", per_path(inputs), True, bands=bands)
    for key in got:
        assert same_bits(cut[key], got[key]), (name, key)


@pytest.mark.parametrize("from_last", [False, True])
def test_values_chosen_for_the_branches(engine, from_last):
    """Rayleigh scattering alone over beta = 0 (exactly conservative), k2*(1 + t*t) on both sides
    of 1e-10, s*beta >= 800, s_l = 0 levels, a thick conservative atmosphere, omega = 0; a grey
    scatterer with omega_c = 0 and 1 and g_c up to 0.9; k*mu0 = 1 + d around the resonance guard."""
    ro = ts.rayleigh_only()
    got = run(engine, ro, "padded", per_path(ro), from_last)
    check(("rayleigh only", from_last), ro, got, from_last)
    f0 = ro.f0()
    # Nothing is absorbed in the columns without an absorber: under A = 1 all of F0 comes back.
    clear = (ro.group == 0) | (ro.group == 4)
    assert np.all(np.abs(got["top_up"][0][clear].astype(LD) - f0[0][clear]) <=
                  FLUX_BOUND*f0[0][clear])
    # Without scattering nothing diffuse comes down, and S = 0 gives 0 everywhere.
    assert np.all(got["diffuse"][:, ro.group == 5] == 0.)
    dark = ro.solar == 0.
    assert np.any(dark) and all(np.all(got[name][:, dark] == 0.) for name in NAMES)
    # s*beta >= 800 in the level nearest space: nothing of the beam is left below it.
    assert np.all(got["direct"][:, ro.group == 2] == 0.)

    cloud = ts.cloud()
    got = run(engine, cloud, "offset", whole(cloud), from_last)
    check(("cloud", from_last), cloud, got, from_last)
    # The same without the sigma row where no level has an air column.
    bare = ts.cloud()
    bare.table[:, 1] = 0.
    with_row = run(engine, bare, "aligned", whole(bare), from_last)
    without = run(engine, bare, "aligned", whole(bare), from_last, sigma=False)
    for key in with_row:
        assert same_bits(with_row[key], without[key]), key

    res = ts.resonance()
    got = run(engine, res, "exact", whole(res), from_last)
    check(("resonance", from_last), res, got, from_last)


def test_a_run_touches_only_its_paths_and_wanted_rows(engine):
    inputs = ts.shape_inputs(131, 5, 3)
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
# lbl_rayleigh_row.
def test_rayleigh_row(engine):
    nu = ts.rayleigh_grid()
    reference, x = ts.rayleigh(LD, nu)
    grid = engine.load_grid(nu)
    try:
        for layout in ("aligned", "offset"):
            row = block(None, 1, nu.size, layout, SENTINEL)
            ordered(engine)
            engine.rayleigh_row(grid, Rows(row), nu.size)
            engine.synchronize()
            got = read(row, nu.size)[0]
            assert np.all(got[:2] == 0.) and np.all(got[2:] > 0.) and np.all(np.isfinite(got))
            error = np.abs(got.astype(LD) - reference)
            allowed = (4*x + 4)*LD(2.**-53)*reference
            print("rayleigh row, %s: worst error / bound %.3g" % (
                layout, float(np.max(error[2:]/allowed[2:]))))
            assert np.all(error <= allowed), layout
            values = np.random.default_rng(8).uniform(0., 1e-29, size=nu.size)
            values[::9] = 0.
            engine.rayleigh_row(grid, Rows(row), nu.size, cross_section=values)
            engine.synchronize()
            assert same_bits(read(row, nu.size)[0], values), layout
        from pylbl_amd.engine import EngineError
        row = block(None, 1, nu.size, "aligned", SENTINEL)
        for values in (np.where(np.arange(nu.size) == 5, -1e-30, 1e-30),
                       np.where(np.arange(nu.size) == 7, np.nan, 1e-30),
                       np.where(np.arange(nu.size) == 7, np.inf, 1e-30)):
            with pytest.raises(EngineError, match="lbl_rayleigh_row"):
                engine.rayleigh_row(grid, Rows(row), nu.size, cross_section=values)
        with pytest.raises(EngineError, match="lbl_rayleigh_row"):
            engine.rayleigh_row(grid + 1000, Rows(row), nu.size)
        engine.synchronize()
        assert np.all(read(row) == SENTINEL)
    finally:
        engine.free_grid(grid)


# ---------------------------------------------------------------------------------------------
# Refused calls.
def test_rejected_calls_write_nothing(engine):
    from pylbl_amd.engine import EngineError, PATH_CONTINUE
    inputs = ts.shape_inputs(67, 3, 1)
    columns, levels = inputs.columns, inputs.levels

    def blocks():
        made = {"beta": block(inputs.beta, levels, columns, "aligned", np.nan),
                "solar": block(inputs.solar[None, :], 1, columns, "aligned", np.nan),
                "sigma": block(inputs.sigma[None, :], 1, columns, "aligned", np.nan),
                "work": block(None, 2*levels, columns, "aligned", SENTINEL)}
        for name in NAMES:
            made[name] = block(None, PATHS if name.startswith("top_") else levels, columns,
                               "aligned", SENTINEL)
        return made

    def changed(row, column, value):
        table = inputs.table.copy()
        table[row, column] = value
        return table

    good = dict(table=inputs.table, mu0=inputs.mu0, albedo=inputs.albedo, albedo_rows=False,
                first=0, count=levels, outputs=NAMES, alias=None)
    bad = [dict(table=changed(4, 0, np.nan)), dict(table=changed(4, 0, -1.)),
           dict(table=changed(2, 1, np.inf)), dict(table=changed(2, 2, -0.5)),
           dict(table=changed(5, 3, 1e3)),                      # w_c > tau_c
           dict(table=changed(5, 4, 1e3)),                      # h_c > w_c
           dict(mu0=np.array([1., 0., 0.5])), dict(mu0=np.array([1., 1.5, 0.5])),
           dict(mu0=np.array([1., np.nan, 0.5])),
           dict(albedo=None),                                   # no albedo at all
           dict(albedo_rows=True),                              # both albedos
           dict(albedo=np.array([0., 1.2, 0.5])),
           dict(first=0, count=4), dict(first=3, count=5),      # runs that cut a path
           dict(first=1, count=3),
           dict(outputs=()), dict(alias="beta"), dict(alias="work")]
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
        with pytest.raises(EngineError, match="lbl_path_two_stream"):
            engine.path_two_stream(
                Rows(made["beta"][part]), columns, PATHS, 3, first, case["table"][part],
                case["mu0"], Rows(made["solar"]), Rows(made["work"][:2*count]),
                rayleigh_row=Rows(made["sigma"]), albedo=case["albedo"],
                albedo_rows=Rows(made["up"][:PATHS]) if case["albedo_rows"] else None, **outputs)
        engine.synchronize()
        for name in ("work",) + NAMES:
            assert np.all(read(made[name]) == SENTINEL), (change, name)
    # On the C entry itself (the binding refuses some of these first): a band mean without bands,
    # one without its rows, and a flag of the other sweeps.
    made = blocks()
    mean = plain(levels, 2)
    bands = np.array([0, 5, 67], dtype=np.int64)

    def raw(n_bands, band_start, rows, means, flags):
        pointers = [None]*16
        for index in rows:
            pointers[index] = made["up"].data_ptr()
        for index in means:
            pointers[8 + index] = mean.data_ptr()
        return engine.lib.lbl_path_two_stream(
            engine.handle, made["beta"].data_ptr(), made["beta"].shape[1], columns, PATHS, 3, 0,
            levels, inputs.table.ctypes.data, inputs.mu0.ctypes.data, made["solar"].data_ptr(),
            None, None, inputs.albedo.ctypes.data, n_bands, band_start, made["work"].data_ptr(),
            *pointers, flags)

    ordered(engine)
    for arguments in ((0, None, [0], [0], 0), (2, bands.ctypes.data, [0], [1], 0),
                      (0, None, [0], [], PATH_CONTINUE)):
        assert raw(*arguments) != 0, arguments
        assert b"lbl_path_two_stream" in engine.lib.lbl_last_error(engine.handle)
    engine.synchronize()
    for name in ("work",) + NAMES:
        assert np.all(read(made[name]) == SENTINEL), name
    assert np.all(read(mean) == SENTINEL)
    # The same call without the fault is taken.
    assert raw(2, bands.ctypes.data, [0], [0], 0) == 0
    engine.synchronize()
    assert np.all(np.isfinite(read(mean))) and np.all(read(made["up"], columns) != SENTINEL)
