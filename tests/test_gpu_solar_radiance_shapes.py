"""lbl_path_solar_radiance fed directly (Engine.path_solar_radiance on rows held in torch tensors),
with flux rows made by the numpy mirror so that the kernel is tested alone, at the shapes
Spectroscopy never gives it: 1, kPathWidth - 1, kPathWidth + 1 and kPathThreads*kPathWidth + 1
columns on layouts that force both kVector instantiations (odd strides, bases that are not 16-byte
aligned, NaN in the padding), 1, 2 and kPathAhead + 1 levels per path, both storage orders, three
paths that differ in mu, mu0 and phi and one path alone, scalar and spectral albedo, runs of whole
paths, bands, the values chosen for the branches of the level (tests/test_solar_radiance_host.py
proves on the CPU that the case tables of tests/solar_radiance_cases.py reach them) and calls that
must be refused.

Bounds, none taken from the code under test.  The reference is the long-double mirror of
tests/solar_radiance_cases.py, continued from the float64 layer inputs and fed the same float64
flux rows.  Every radiance is within (4*E_cpu + 1e-13)*scale of it, scale = max(F0/pi, the
long-double mirror's largest |I| at the path's interfaces): E_cpu = 7.9e-12 is the worst |float64
mirror - long-double mirror|/scale that tests/test_solar_radiance_host.py measures over the same
case tables (recorded as solar_radiance_cases.E_CPU = 8e-12, capped at 1e-10); the factor 4 because
the device's exp and expm1 are a few ulp where numpy's are about one.  Band means are within 1e-12
* magnitude of the long-double means of the rows the call itself wrote.  Nothing is NaN or inf.
All layouts of a case, and all cuts into runs of whole paths, give identical bits; beta and the
flux rows are unwritten."""
import numpy as np
import pytest

from tests import solar_radiance_cases as sc
from tests import sweep_cases as cases
from tests import two_stream_cases as ts
from tests.test_gpu_sweep_shapes import Rows, block, ordered, plain, read, same_bits

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
BOUND = LD(4.*sc.E_CPU + sc.FLOOR)
MEAN_BOUND = LD(1e-12)
MU, PHI = np.array(sc.MU), np.array(sc.PHI)
PATH_WIDTH, PATH_THREADS = 2, 256       # kPathWidth, kPathThreads
COLUMNS = (1, PATH_WIDTH + 1, PATH_THREADS*PATH_WIDTH + 1)
FLUXES = ("up", "direct", "diffuse")
WORST = [0.]


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    yield default_engine(0)
    print("\nworst error / bound, solar_view_kernel: %.3g" % WORST[0])


def run(engine, inputs, mu, phi, layout, runs, from_last, bands=None, fluxes=None, paths=PATHS,
        fill=SENTINEL):
    """The outputs of the entry over `runs` of whole paths (first level, count) of the first
    `paths` paths."""
    n, columns = inputs.levels_per_path, inputs.columns
    levels = paths*n
    fluxes = sc.flux_rows(inputs, from_last) if fluxes is None else fluxes
    cos_theta = sc.scattering_cosine(mu, inputs.mu0, phi)
    beta = block(inputs.beta[:levels], levels, columns, layout, np.nan)
    rows = {q: block(fluxes[q][:levels], levels, columns, layout, np.nan) for q in FLUXES}
    solar = block(inputs.solar[None, :], 1, columns, layout, np.nan)
    sigma = block(inputs.sigma[None, :], 1, columns, layout, np.nan)
    radiance = block(None, paths, columns, layout, fill)
    mean = None if bands is None else plain(paths, bands.size - 1)
    keywords = {}
    if inputs.albedo.ndim == 2:
        keywords["albedo_rows"] = Rows(block(inputs.albedo[:paths], paths, columns, layout, np.nan))
    else:
        keywords["albedo"] = inputs.albedo[:paths]
    ordered(engine)
    for first, count in runs:
        part = slice(first, first + count)
        outputs = {"radiance_rows": Rows(radiance)}
        if bands is not None:
            outputs["radiance_mean"] = Rows(mean)
        engine.path_solar_radiance(
            Rows(beta[part]), columns, paths, n, first, inputs.table[part], inputs.mu0[:paths],
            mu[:paths], cos_theta[:paths], Rows(solar), Rows(rows["up"][part]),
            Rows(rows["direct"][part]), Rows(rows["diffuse"][part]), rayleigh_row=Rows(sigma),
            band_start=bands, from_last=from_last, **outputs, **keywords)
        engine.synchronize()
    host = radiance.cpu().numpy()
    if np.isnan(fill):
        assert np.all(np.isnan(host[:, columns:])), "the padding of the output was written"
    else:
        assert np.all(host[:, columns:] == fill), "the padding of the output was written"
    out = {"radiance": np.ascontiguousarray(host[:, :columns])}
    if mean is not None:
        out["radiance mean"] = read(mean)
    assert np.array_equal(read(beta)[:, :columns], inputs.beta[:levels]), "beta was written"
    for q in FLUXES:
        assert same_bits(read(rows[q])[:, :columns], fluxes[q][:levels]), q + "_rows were written"
    return out


def reference(inputs, mu, phi, from_last):
    """The long-double mirror of a problem, formed once."""
    store = inputs.__dict__.setdefault("_view", {})
    key = (tuple(mu), tuple(phi), from_last)
    if key not in store:
        fluxes = sc.flux_rows(inputs, from_last)
        cos_theta = sc.scattering_cosine(mu, inputs.mu0, phi)
        high = sc.mirror(LD, inputs, mu, cos_theta, from_last, fluxes)
        store[key] = (fluxes, high, sc.scale(inputs, high))
    return store[key]


def check(what, inputs, mu, phi, got, from_last, bands=None):
    """Every radiance within BOUND*scale of the long-double mirror, finite and, where the Sun is
    dark, 0."""
    _, expect, scale = reference(inputs, mu, phi, from_last)
    value = got["radiance"]
    rows = value.shape[0]
    assert np.all(np.isfinite(value)), what
    error = np.abs(value.astype(LD) - expect["radiance"][:rows])
    allowed = BOUND*scale[:rows]
    lit = allowed > 0.
    worst = float(np.max(error[lit]/allowed[lit], initial=0.))
    WORST[0] = max(WORST[0], worst)
    print("%s: worst error / bound %.3g" % (what, worst))
    assert np.all(error <= allowed), (what, worst)
    if bands is not None:
        means = cases.band_means(LD, value, bands)
        mean = got["radiance mean"]
        empty = np.isnan(means)
        assert np.array_equal(np.isnan(mean), empty) and np.count_nonzero(~empty), what
        assert np.any(empty), "no empty band"
        assert np.all(np.abs(mean[~empty].astype(LD) - means[~empty]) <=
                      MEAN_BOUND*np.abs(means[~empty])), (what, "mean")


def whole(inputs, paths=PATHS):
    return [(0, paths*inputs.levels_per_path)]


def per_path(inputs, reverse=False):
    n = inputs.levels_per_path
    runs = [(p*n, n) for p in range(PATHS)]
    return runs[::-1] if reverse else runs


def shape_inputs(columns, depth, seed, albedo_rows=False):
    return sc.under_sun(ts.shape_inputs(columns, depth, seed, albedo_rows=albedo_rows), sc.MU0)


@pytest.mark.parametrize("columns", COLUMNS)
def test_columns_on_every_layout(engine, columns):
    """Both kVector instantiations: "aligned" takes the vector kernel, an odd stride or a base 8
    bytes off the scalar one."""
    assert cases.layout_is_vector("aligned", columns)
    assert not cases.layout_is_vector("odd", columns)
    assert not cases.layout_is_vector("offset", columns)
    inputs = shape_inputs(columns, 9, columns)
    base = None
    for layout in cases.LAYOUTS:
        got = run(engine, inputs, MU, PHI, layout, whole(inputs), True)
        if base is None:
            base = got
            check((columns, layout), inputs, MU, PHI, got, True)
        assert same_bits(got["radiance"], base["radiance"]), (columns, layout)


@pytest.mark.parametrize("depth", sc.DEPTHS)
@pytest.mark.parametrize("from_last", [False, True])
def test_depths_both_orders_runs_and_spectral_albedo(engine, depth, from_last):
    inputs = shape_inputs(513, depth, 40 + depth, albedo_rows=True)
    base = None
    for layout, runs in (("aligned", whole(inputs)), ("odd", per_path(inputs, from_last)),
                         ("aligned", per_path(inputs, not from_last))):
        got = run(engine, inputs, MU, PHI, layout, runs, from_last)
        if base is None:
            base = got
            check((depth, from_last, layout), inputs, MU, PHI, got, from_last)
        assert same_bits(got["radiance"], base["radiance"]), (depth, from_last, layout)


def test_one_path_alone_and_scalar_albedo_as_its_row(engine):
    """Three paths that differ in mu, mu0 and phi; the first of them alone in a call of one path;
    A = (1, 0.3, 0) as scalars and as rows."""
    inputs = shape_inputs(131, 2, 3)
    assert tuple(inputs.albedo) == (1., 0.3, 0.)
    assert len(set(MU)) == len(set(inputs.mu0)) == len(set(PHI)) == PATHS
    three = run(engine, inputs, MU, PHI, "aligned", whole(inputs), False)
    check("three paths", inputs, MU, PHI, three, False)
    one = run(engine, inputs, MU, PHI, "offset", whole(inputs, 1), False, paths=1)
    assert one["radiance"].shape == (1, 131)
    assert same_bits(one["radiance"], three["radiance"][:1])
    rows = shape_inputs(131, 2, 3)
    rows.albedo = np.repeat(inputs.albedo[:, None], 131, axis=1)
    spectral = run(engine, rows, MU, PHI, "odd", whole(rows), False)
    assert same_bits(three["radiance"], spectral["radiance"])


@pytest.mark.parametrize("name, columns, bands", cases.BAND_SETS)
def test_band_means(engine, name, columns, bands):
    inputs = shape_inputs(columns, 3, 70)
    got = run(engine, inputs, MU, PHI, "aligned", whole(inputs), True, bands=bands)
    check(name, inputs, MU, PHI, got, True, bands=bands)
    cut = run(engine, inputs, MU, PHI, "padded", per_path(inputs), True, bands=bands)
    for key in got:
        assert same_bits(cut[key], got[key]), (name, key)


@pytest.mark.parametrize("from_last", [False, True])
def test_values_chosen_for_the_branches(engine, from_last):
    """Rayleigh only (the identity level, both sides of the conservative threshold), clouds,
    levels inside the guard k*mu0 = 1, a conservative cloud, k*mu = 1 exactly and 1 +- 1e-9 and
    k*t = 1000, under every pair of mu and mu0."""
    layouts = ("padded", "offset", "exact", "aligned", "odd")
    for index, (inputs, mu, phi) in enumerate(sc.value_cases()):
        layout = layouts[index % len(layouts)]
        runs = per_path(inputs) if layout == "padded" else whole(inputs)
        got = run(engine, inputs, mu, phi, layout, runs, from_last)
        check((inputs.name, from_last, tuple(mu)), inputs, mu, phi, got, from_last)


def test_poisoned_output_rows_are_overwritten_on_the_columns_alone(engine):
    """NaN in the output before the call: every column of every path is written, nothing beyond
    the columns (run() checks the padding), and a run writes only its own paths."""
    inputs = shape_inputs(131, 2, 3)
    n = inputs.levels_per_path
    everything = run(engine, inputs, MU, PHI, "padded", whole(inputs), False, fill=np.nan)
    assert np.all(np.isfinite(everything["radiance"]))
    check("poisoned", inputs, MU, PHI, everything, False)
    middle = run(engine, inputs, MU, PHI, "padded", [(n, n)], False, fill=np.nan)
    assert same_bits(middle["radiance"][1], everything["radiance"][1])
    assert np.all(np.isnan(middle["radiance"][[0, 2]]))


# ---------------------------------------------------------------------------------------------
# Refused calls.
def test_rejected_calls_write_nothing_and_leave_the_engine_usable(engine):
    from pylbl_amd.engine import EngineError, PATH_CONTINUE
    inputs = shape_inputs(67, 3, 1)
    columns, levels = inputs.columns, inputs.levels
    fluxes = sc.flux_rows(inputs, False)
    cos_theta = sc.scattering_cosine(MU, inputs.mu0, PHI)
    inputs_rows = ("beta", "up", "direct", "diffuse", "solar", "sigma")

    def blocks():
        made = {"beta": block(inputs.beta, levels, columns, "aligned", np.nan),
                "solar": block(inputs.solar[None, :], 1, columns, "aligned", np.nan),
                "sigma": block(inputs.sigma[None, :], 1, columns, "aligned", np.nan)}
        for q in FLUXES:
            made[q] = block(fluxes[q], levels, columns, "aligned", np.nan)
        for name in ("radiance", "spare"):
            made[name] = block(None, levels, columns, "aligned", SENTINEL)
        return made

    def changed(row, column, value):
        table = inputs.table.copy()
        table[row, column] = value
        return table

    def untouched(made, change):
        for name in ("radiance", "spare"):
            assert np.all(read(made[name]) == SENTINEL), (change, name)
        assert np.array_equal(read(made["beta"])[:, :columns], inputs.beta), change
        for q in FLUXES:
            assert same_bits(read(made[q])[:, :columns], fluxes[q]), (change, q)
        assert same_bits(read(made["solar"])[0, :columns], inputs.solar), change
        assert same_bits(read(made["sigma"])[0, :columns], inputs.sigma), change

    cloudy = int(np.flatnonzero(inputs.table[:, 3] > 0.)[0])
    good = dict(table=inputs.table, mu0=inputs.mu0, albedo=inputs.albedo, albedo_rows=False,
                first=0, count=levels, alias=None, mu=MU, cos_theta=cos_theta, output=True)
    bad = [dict(table=changed(4, 0, np.nan)), dict(table=changed(4, 0, -1.)),
           dict(table=changed(2, 1, np.inf)), dict(table=changed(2, 2, -0.5)),
           dict(table=changed(cloudy, 3, 1e3)),                 # w_c > tau_c
           dict(table=changed(cloudy, 4, 1e3)),                 # h_c > w_c
           dict(table=changed(cloudy, 4, inputs.table[cloudy, 3])),     # g_c = 1
           dict(mu0=np.array([1., 0., 0.5])), dict(mu0=np.array([1., 1.0001, 0.5])),
           dict(mu0=np.array([np.nan, 1., 0.5])),
           dict(albedo=None),                                   # no albedo at all
           dict(albedo_rows=True),                              # both albedos
           dict(albedo=np.array([0., 1.2, 0.5])), dict(albedo=np.array([0., -0.1, 0.5])),
           dict(mu=np.array([1., 0., 0.5])), dict(mu=np.array([1., 1.0001, 0.5])),
           dict(mu=np.array([1., -0.5, 0.5])), dict(mu=np.array([np.nan, 1., 0.5])),
           dict(mu=np.array([1., 1., np.inf])),
           dict(cos_theta=np.array([0., 1.0001, 0.5])), dict(cos_theta=np.array([-1.0001, 0., 0.])),
           dict(cos_theta=np.array([0., np.nan, 0.5])), dict(cos_theta=np.array([0., 0., np.inf])),
           dict(first=0, count=4), dict(first=3, count=5),      # runs that cut a path
           dict(first=1, count=3),
           dict(output=False)] + [dict(alias=name) for name in inputs_rows]
    for change in bad:
        case = dict(good, **change)
        made = blocks()
        first, count = case["first"], case["count"]
        part = slice(first, first + count)
        outputs = {"radiance_rows": Rows(made["radiance"][:PATHS])} if case["output"] else {}
        if case["alias"] is not None:
            alias = made[case["alias"]]
            outputs["radiance_rows"] = Rows(alias[part] if alias.shape[0] == levels else alias)
        ordered(engine)
        with pytest.raises((EngineError, ValueError), match="lbl_path_solar_radiance|an output"):
            engine.path_solar_radiance(
                Rows(made["beta"][part]), columns, PATHS, 3, first, case["table"][part],
                case["mu0"], case["mu"], case["cos_theta"], Rows(made["solar"]),
                Rows(made["up"][part]), Rows(made["direct"][part]), Rows(made["diffuse"][part]),
                rayleigh_row=Rows(made["sigma"]), albedo=case["albedo"],
                albedo_rows=Rows(made["spare"][:PATHS]) if case["albedo_rows"] else None,
                **outputs)
        engine.synchronize()
        untouched(made, change)
    # On the C entry itself (the binding refuses some of these first): a missing flux row, an
    # output that is an input row, a band mean without bands, one without its rows, and a flag of
    # the other sweeps.
    made = blocks()
    mean = plain(PATHS, 2)
    bands = np.array([0, 5, 67], dtype=np.int64)

    def raw(n_bands, band_start, up, direct, diffuse, radiance, means, flags):
        pointer = lambda name: made[name].data_ptr() if name else None      # noqa: E731
        return engine.lib.lbl_path_solar_radiance(
            engine.handle, made["beta"].data_ptr(), made["beta"].shape[1], columns, PATHS, 3, 0,
            levels, inputs.table.ctypes.data, inputs.mu0.ctypes.data, MU.ctypes.data,
            cos_theta.ctypes.data, made["solar"].data_ptr(), made["sigma"].data_ptr(), None,
            inputs.albedo.ctypes.data, pointer(up), pointer(direct), pointer(diffuse), n_bands,
            band_start, pointer(radiance), mean.data_ptr() if means else None, flags)

    ordered(engine)
    for arguments in ((0, None, None, "direct", "diffuse", "radiance", False, 0),
                      (0, None, "up", None, "diffuse", "radiance", False, 0),
                      (0, None, "up", "direct", None, "radiance", False, 0),
                      (0, None, "up", "direct", "diffuse", "solar", False, 0),
                      (0, None, "up", "direct", "diffuse", "sigma", False, 0),
                      (0, None, "up", "direct", "diffuse", "radiance", True, 0),
                      (2, bands.ctypes.data, "up", "direct", "diffuse", None, True, 0),
                      (0, None, "up", "direct", "diffuse", "radiance", False, PATH_CONTINUE)):
        assert raw(*arguments) != 0, arguments
        assert b"lbl_path_solar_radiance" in engine.lib.lbl_last_error(engine.handle)
    engine.synchronize()
    untouched(made, "raw")
    assert np.all(read(mean) == SENTINEL)
    # The same call without the fault is taken: the engine is usable.
    assert raw(2, bands.ctypes.data, "up", "direct", "diffuse", "radiance", True, 0) == 0
    engine.synchronize()
    assert np.all(np.isfinite(read(mean)))
    assert np.all(read(made["radiance"], columns)[:PATHS] != SENTINEL)
    assert np.all(read(made["radiance"])[PATHS:] == SENTINEL)
