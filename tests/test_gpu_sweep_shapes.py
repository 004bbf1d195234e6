"""lbl_path_compute, lbl_path_radiance and lbl_path_flux fed directly (Engine.path_compute /
path_radiance / path_flux on rows held in torch tensors) at the shapes Spectroscopy never gives
them: odd strides and bases that are not 16-byte aligned (the scalar kernels), one-column tail
lanes, NaN in the padding, every depth of path_levels' rows-in-flight loop with every (starts,
finishes) pair, every K, band segments at their edges, and values chosen for the arithmetic.
tests/test_sweep_host.py proves on the CPU that the case tables of tests/sweep_cases.py reach
those code paths.

Bounds, none taken from the code under test: tau is the float64 numpy loop bit for bit (the header's
contract); exp(-tau) is within 1e-15 relative of the long-double exp of that tau (what
test_gpu_path.py's test_large_grid asserts); radiance, brightness temperature, flux and every band
mean are within 1e-12 * magnitude of the long-double recurrence, the magnitude being the same
recurrence over absolute values (for beta >= 0 the value itself: the 1e-12 relative bound of
test_gpu_radiance.py and test_gpu_flux.py).  Layouts and runs of one case give the same bits."""
import numpy as np
import pytest

from tests import sweep_cases as cases

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
BOUND, TRANS_BOUND = LD(1e-12), LD(1e-15)
WORST = {}      # kernel -> worst observed error / bound


class Rows(object):
    """A float64 torch tensor [rows, row stride] on the GPU, as the engine's beta, carry or out."""
    def __init__(self, tensor):
        assert tensor.dtype.is_floating_point and tensor.dim() == 2
        assert tensor.stride(1) == 1 and tensor.stride(0) == tensor.shape[1]
        self.tensor = tensor
        self.pointer, self.shape = tensor.data_ptr(), tuple(tensor.shape)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    yield default_engine(0)
    for kernel, ratio in sorted(WORST.items()):
        print("\nworst error / bound, %s: %.3g" % (kernel, ratio))


def block(values, rows, columns, layout, fill):
    """[rows, stride] on the GPU in `layout`: `values` [rows, columns] (None: `fill`) in the first
    `columns` values of each row, `fill` in the padding."""
    import torch
    layout = cases.LAYOUTS[layout]
    stride = layout.stride(columns)
    host = np.full((rows, stride), fill, dtype=F64)
    if values is not None:
        host[:, :columns] = values
    flat = torch.full((rows*stride + 2,), fill, dtype=torch.float64, device="cuda:0")
    view = flat[layout.offset:layout.offset + rows*stride].view(rows, stride)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == 8*(layout.offset % 2)
    return view


def plain(rows, width):
    import torch
    return torch.full((rows, width), SENTINEL, dtype=torch.float64, device="cuda:0")


def read(tensor, columns=None):
    """The tensor on the host, its padding checked to be untouched."""
    host = tensor.cpu().numpy()
    if columns is None:
        return host
    assert np.all(host[:, columns:] == SENTINEL), "the padding of an output was written"
    return np.ascontiguousarray(host[:, :columns])


def ordered(engine):
    import torch
    engine.order_after_stream(torch.cuda.current_stream("cuda:0").cuda_stream)


def unfinished(first, count, n, from_last):
    """(path, flat level) the run leaves inside a path in sweep order, or None."""
    if from_last:
        return (first//n, first) if first % n else None
    end = first + count
    return (end//n, end - 1) if end % n else None


def in_order(runs, from_last):
    return list(reversed(runs)) if from_last else list(runs)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F64), np.ascontiguousarray(b, dtype=F64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_same(got, base, what):
    """Every output the two results share, bit for bit."""
    shared = [k for k in got if k in base]
    assert shared and all(k in got for k in base if "@" not in k), what
    for key in shared:
        assert same_bits(got[key], base[key]), (what, key)


# ---------------------------------------------------------------------------------------------
# Comparisons.
def close(kernel, what, got, reference, magnitude, bound=BOUND):
    """|got - reference| <= bound*magnitude wherever the reference is a number, NaN exactly where
    it is NaN (empty bands), never inf; at least one number is compared."""
    got = np.asarray(got, dtype=F64)
    reference = cases.flushed(np.asarray(reference, dtype=LD))
    magnitude = np.broadcast_to(np.asarray(magnitude, dtype=LD), reference.shape)
    assert got.shape == reference.shape and got.size > 0, what
    empty = np.isnan(reference)
    assert np.array_equal(np.isnan(got), empty), what
    assert not np.any(np.isinf(got)), what
    ok = ~empty
    assert np.count_nonzero(ok) > 0, what
    error = np.abs(got[ok].astype(LD) - reference[ok])
    allowed = bound*magnitude[ok]
    scaled = allowed > 0.
    ratio = float(np.max(error[scaled]/allowed[scaled], initial=0.))
    WORST[kernel] = max(WORST.get(kernel, 0.), ratio)
    assert np.all(error <= allowed), (what, ratio, float(np.max(error[~scaled], initial=0.)))


def cached(problem, key, sweep):
    """The reference sweeps of a problem, formed once."""
    store = problem.__dict__.setdefault("_sweeps", {})
    if key not in store:
        store[key] = sweep()
    return store[key]


def bits(kernel, what, got, loop):
    assert got.size > 0 and same_bits(got, loop), what


def check(kernel, what, got, expect):
    """expect: {key: ("bits", loop) | ("close", reference, magnitude[, bound])}; every key of
    `got` is checked."""
    assert set(got) == set(expect), (what, sorted(set(got) ^ set(expect)))
    for key, rule in expect.items():
        if rule[0] == "bits":
            bits(kernel, (what, key), got[key], rule[1])
        else:
            close(kernel, (what, key), got[key], *rule[1:])


# ---------------------------------------------------------------------------------------------
# lbl_path_compute.
PATH_MODES = ("per path", "cumulative", "bands", "cumulative bands")


def run_path(engine, problem, layout, runs, mode, from_last=False, bands=None):
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    cumulative = mode.startswith("cumulative")
    with_bands = mode.endswith("bands")
    assert with_bands == (bands is not None) and (cumulative or not from_last)
    beta = block(problem.beta, levels, columns, layout, np.nan)
    carry = block(None, PATHS, columns, layout, SENTINEL)
    rows = levels if cumulative else PATHS
    if with_bands:
        tau, trans = plain(rows, bands.size - 1), plain(rows, bands.size - 1)
    else:
        tau = block(None, rows, columns, layout, SENTINEL)
        trans = block(None, rows, columns, layout, SENTINEL)
    out = {}
    ordered(engine)
    for first, count in in_order(runs, from_last):
        part = slice(first, first + count)
        engine.path_compute(Rows(beta[part]), columns, PATHS, n, first, problem.thickness[part],
                            Rows(carry), optical_depth=Rows(tau[part] if cumulative else tau),
                            transmittance=Rows(trans[part] if cumulative else trans),
                            band_start=bands, cumulative=cumulative, from_last=from_last)
        engine.synchronize()
        left = unfinished(first, count, n, from_last)
        if left is not None:
            out["carry@%d" % left[1]] = read(carry, columns)[left[0]]
    if with_bands:
        out["tau mean"], out["trans mean"] = read(tau), read(trans)
        if cumulative:
            out["beta"] = read(beta)[:, :columns]
        else:
            out["carry"] = read(carry, columns)
    else:
        out["tau"], out["trans"] = read(tau, columns), read(trans, columns)
    return out


def expect_path(problem, got, mode, from_last=False, bands=None):
    n = problem.levels_per_path
    def sweep():
        loop, _ = cases.sweep_tau(F64, problem.beta, problem.thickness, n, from_last)
        tau, mag = cases.sweep_tau(LD, problem.beta, problem.thickness, n, from_last)
        with np.errstate(under="ignore", over="ignore"):
            return loop, tau, mag, np.exp(-loop.astype(LD))
    loop, tau, mag, trans = cached(problem, ("path", from_last), sweep)
    rows = slice(None) if mode.startswith("cumulative") else cases._flat(n, n - 1)
    expect = {k: ("bits", loop[int(k.split("@")[1])]) for k in got if "@" in k}
    if bands is None:
        expect["tau"] = ("bits", loop[rows])
        expect["trans"] = ("close", trans[rows], trans[rows], TRANS_BOUND)
    else:
        expect["tau mean"] = ("close", cases.band_means(LD, tau[rows], bands),
                              cases.band_means(LD, mag[rows], bands))
        mean = cases.band_means(LD, trans[rows], bands)
        expect["trans mean"] = ("close", mean, mean)
        expect["beta" if mode.startswith("cumulative") else "carry"] = ("bits", loop[rows])
    return expect


# ---------------------------------------------------------------------------------------------
# lbl_path_radiance.
def run_radiance(engine, grid, problem, layout, runs, mode, from_last=False, bands=None,
                 boundary=True):
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    cumulative = mode.startswith("cumulative")
    with_bands = mode.endswith("bands")
    assert with_bands == (bands is not None)
    beta = block(problem.beta, levels, columns, layout, np.nan)
    carry = block(None, PATHS, columns, layout, SENTINEL)
    rows = levels if cumulative else PATHS
    if with_bands:
        rad, bt = plain(rows, bands.size - 1), None
    else:
        rad = block(None, rows, columns, layout, SENTINEL)
        bt = block(None, rows, columns, layout, SENTINEL)
    out = {}
    ordered(engine)
    for first, count in in_order(runs, from_last):
        part = slice(first, first + count)
        engine.path_radiance(
            Rows(beta[part]), columns, grid, PATHS, n, first, problem.thickness[part],
            problem.temperature[part], Rows(carry),
            boundary_temperature=problem.boundary_t if boundary else None,
            boundary_emissivity=problem.boundary_e if boundary else None,
            radiance=Rows(rad[part] if cumulative else rad),
            brightness_temperature=None if bt is None else Rows(bt[part] if cumulative else bt),
            band_start=bands, cumulative=cumulative, from_last=from_last)
        engine.synchronize()
        left = unfinished(first, count, n, from_last)
        if left is not None:
            out["carry@%d" % left[1]] = read(carry, columns)[left[0]]
    if with_bands:
        out["rad mean"] = read(rad)
        if cumulative:
            out["beta"] = read(beta)[:, :columns]
        else:
            out["carry"] = read(carry, columns)
    else:
        out["rad"], out["bt"] = read(rad, columns), read(bt, columns)
    return out


def expect_radiance(problem, got, mode, from_last=False, bands=None, boundary=True):
    n, nu = problem.levels_per_path, problem.nu
    start = cases.boundary_start(LD, nu, problem.boundary_t, problem.boundary_e) \
        if boundary else None
    rad, mag = cached(problem, ("radiance", from_last, boundary), lambda: cases.sweep_radiance(
        LD, nu, problem.beta, problem.thickness, problem.temperature, n, from_last, start))
    rows = slice(None) if mode.startswith("cumulative") else cases._flat(n, 0 if from_last
                                                                         else n - 1)
    expect = {k: ("close", rad[int(k.split("@")[1])], mag[int(k.split("@")[1])])
              for k in got if "@" in k}
    if bands is None:
        flushed = cases.flushed(rad[rows])
        expect["rad"] = ("close", rad[rows], mag[rows])
        expect["bt"] = ("close", cases.brightness(LD, nu, flushed),
                        cases.brightness_magnitude(LD, nu, flushed, mag[rows]))
    else:
        expect["rad mean"] = ("close", cases.band_means(LD, rad[rows], bands),
                              cases.band_means(LD, mag[rows], bands))
        expect["beta" if mode.startswith("cumulative") else "carry"] = \
            ("close", rad[rows], mag[rows])
    return expect


# ---------------------------------------------------------------------------------------------
# lbl_path_flux: the down sweep, then the up sweep over the same reflection rows.
def run_flux(engine, grid, problem, layout, runs, angles, surface, bands=None):
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    lengths, weight = problem.lengths(angles)
    beta = block(problem.beta, levels, columns, layout, np.nan)
    carry = block(None, PATHS*angles, columns, layout, SENTINEL)
    reflection = block(None, PATHS, columns, layout, SENTINEL)
    out = {}
    ordered(engine)
    for sweep, up in (("down", False), ("up", True)):
        from_last = (surface == "first") != up
        level = block(None, levels, columns, layout, SENTINEL)
        mean = plain(levels, bands.size - 1) if bands is not None else None
        at_surface = plain(PATHS, bands.size - 1) if bands is not None and up else None
        ordered(engine)
        for first, count in in_order(runs, from_last):
            part = slice(first, first + count)
            engine.path_flux(
                Rows(beta[part]), columns, grid, PATHS, n, first, lengths[part], weight,
                problem.temperature[part], Rows(carry), Rows(reflection), Rows(level[part]),
                surface_temperature=problem.surface_t, surface_emissivity=problem.surface_e,
                flux=None if mean is None else Rows(mean[part]),
                surface_flux=None if at_surface is None else Rows(at_surface),
                band_start=bands, up=up, from_last=from_last)
            engine.synchronize()
            left = unfinished(first, count, n, from_last)
            if left is not None:
                rows = slice(left[0]*angles, (left[0] + 1)*angles)
                out["%s carry@%d" % (sweep, left[1])] = read(carry, columns)[rows]
        out[sweep] = read(level, columns)
        out["surface" if up else "reflection"] = read(reflection, columns)
        if mean is not None:
            out[sweep + " mean"] = read(mean)
        if at_surface is not None:
            out["surface mean"] = read(at_surface)
    assert np.all(read(beta)[:, :columns] == problem.beta)      # the block is only read
    return out


def expect_flux(problem, got, angles, surface, bands=None):
    n, nu = problem.levels_per_path, problem.nu
    lengths, weight = problem.lengths(angles)
    down_last = surface == "first"
    def sweep():
        down = cases.sweep_flux(LD, nu, problem.beta, lengths, weight, problem.temperature, n,
                                down_last)
        start, start_mag = cases.surface_start(LD, nu, problem.surface_t, problem.surface_e,
                                               down.total, down.total_mag)
        return down, start, start_mag, cases.sweep_flux(
            LD, nu, problem.beta, lengths, weight, problem.temperature, n, not down_last, start,
            start_mag)
    down, start, start_mag, up = cached(problem, ("flux", angles, surface), sweep)
    w = weight.astype(LD)
    pi = LD(cases.FLUX_PI)
    at_surface = pi*cases.flux_sum(w, np.repeat(start[:, None, :], angles, axis=1))
    at_surface_mag = pi*cases.flux_sum(w, np.repeat(start_mag[:, None, :], angles, axis=1))
    expect = {"down": ("close", down.flux, down.flux_mag), "up": ("close", up.flux, up.flux_mag),
              "reflection": ("close", down.total, down.total_mag),
              "surface": ("close", at_surface, at_surface_mag)}
    for key in got:
        if "@" in key:
            sweep = down if key.startswith("down") else up
            level = int(key.split("@")[1])
            expect[key] = ("close", sweep.rad[level], sweep.rad_mag[level])
    if bands is not None:
        for key, value, mag in (("down mean", down.flux, down.flux_mag),
                                ("up mean", up.flux, up.flux_mag),
                                ("surface mean", at_surface, at_surface_mag)):
            expect[key] = ("close", cases.band_means(LD, value, bands),
                           cases.band_means(LD, mag, bands))
    return expect


# ---------------------------------------------------------------------------------------------
def variants(kernel, bands=None, angles=3):
    """[(name, run(engine, grid, problem, layout, runs), expect(problem, got))] of a kernel: every
    output route, both directions; with `bands` the band-mean routes as well."""
    found = []

    def add(name, run, expect, **keywords):
        found.append((name, lambda e, g, p, layout, runs: run(e, g, p, layout, runs, **keywords),
                      lambda p, got: expect(p, got, **keywords)))

    if kernel == "path":
        def run(e, g, p, layout, runs, **k):
            return run_path(e, p, layout, runs, **k)
        add("per path", run, expect_path, mode="per path")
        for from_last in (False, True):
            add("cumulative %s" % from_last, run, expect_path, mode="cumulative",
                from_last=from_last)
            if bands is not None:
                add("cumulative bands %s" % from_last, run, expect_path,
                    mode="cumulative bands", from_last=from_last, bands=bands)
        if bands is not None:
            add("bands", run, expect_path, mode="bands", bands=bands)
    elif kernel == "radiance":
        for from_last in (False, True):
            for boundary in (True, False):
                mode = "per path" if boundary != from_last else "cumulative"
                add("%s %s %s" % (mode, from_last, boundary), run_radiance, expect_radiance,
                    mode=mode, from_last=from_last, boundary=boundary)
            add("cumulative* %s" % from_last, run_radiance, expect_radiance, mode="cumulative",
                from_last=from_last, boundary=not from_last)
            if bands is not None:
                add("bands %s" % from_last, run_radiance, expect_radiance, mode="bands",
                    from_last=from_last, bands=bands)
                add("cumulative bands %s" % from_last, run_radiance, expect_radiance,
                    mode="cumulative bands", from_last=from_last, bands=bands,
                    boundary=from_last)
    else:
        for surface in ("first", "last"):
            add("surface %s" % surface, run_flux, expect_flux, angles=angles, surface=surface)
            if bands is not None:
                add("surface %s bands" % surface, run_flux, expect_flux, angles=angles,
                    surface=surface, bands=bands)
    return found


class Grid(object):
    def __init__(self, engine, nu):
        self.engine, self.nu = engine, nu

    def __enter__(self):
        self.handle = self.engine.load_grid(self.nu)
        return self.handle

    def __exit__(self, *error):
        self.engine.synchronize()
        self.engine.free_grid(self.handle)


def small_bands(columns):
    """Bands on a small grid: empty ones at 0, inside and at `columns`, the last one ends there."""
    third = columns//3
    return np.array([0, 0, third, third, max(columns - 1, third), columns, columns],
                    dtype=np.int64)


WHOLE = {"whole": None}


@pytest.mark.parametrize("columns", cases.COLUMNS)
@pytest.mark.parametrize("kernel", ["path", "radiance", "flux"])
def test_columns_and_layouts(engine, kernel, columns):
    """9 levels per path (a batch and a remainder) on 1 to 8193 columns: the aligned even-stride
    layout meets the reference, and stride = columns, NaN padding, a base 8 bytes off and an odd
    stride (the scalar kernels, one-column tail lanes) give its bits."""
    problem = cases.Problem(columns, 9, seed=100 + columns)
    runs = cases.run_sets(9)["whole"]
    layouts = [x for x in cases.LAYOUTS if x != "aligned"] if columns in cases.LAYOUT_COLUMNS \
        else []
    bands = small_bands(columns)
    with Grid(engine, problem.nu) as grid:
        for name, run, expect in variants(kernel, bands):
            base = run(engine, grid, problem, "aligned", runs)
            check(kernel, (kernel, columns, name), base, expect(problem, base))
            for layout in layouts:
                assert_same(run(engine, grid, problem, layout, runs), base,
                            (kernel, columns, name, layout))
    print("worst error / bound so far:", WORST)


def run_case_ids():
    return [(kernel, n, angles) for kernel in ("path", "radiance", "flux")
            for n, angles, _ in cases.run_cases(kernel)]


@pytest.mark.parametrize("kernel,n,angles", run_case_ids())
def test_levels_and_runs(engine, kernel, n, angles):
    """Every run set of the case (the whole atmosphere, one level per call, uneven runs, and for
    the deep cases the splits that put every (starts, finishes) pair at every depth of
    path_levels) gives the bits of the single call, carry rows between runs meet the reference,
    and the single call meets it; on a vector and on a scalar layout."""
    sets = [s for m, a, s in cases.run_cases(kernel) if m == n and a == angles][0]
    problem = cases.Problem(cases.RUN_COLUMNS, n, seed=200 + n)
    bands = small_bands(problem.columns)
    deep = len(sets) > 4
    with Grid(engine, problem.nu) as grid:
        for name, run, expect in variants(kernel, bands, angles or 3):
            base = run(engine, grid, problem, "aligned", sets["whole"])
            check(kernel, (kernel, n, name), base, expect(problem, base))
            for layout in ("aligned", "odd") if deep else ("aligned",):
                for run_name, runs in sets.items():
                    if run_name == "whole" and layout == "aligned":
                        continue
                    got = run(engine, grid, problem, layout, runs)
                    assert_same(got, base, (kernel, n, name, layout, run_name))
                    between = {k: v for k, v in got.items() if "@" in k}
                    rules = expect(problem, between)
                    check(kernel, (kernel, n, name, layout, run_name), between,
                          {k: rules[k] for k in between})
    print("worst error / bound so far:", WORST)


@pytest.mark.parametrize("angles", cases.ANGLES)
def test_every_angle_count(engine, angles):
    """K = 1..8 with Gauss-Legendre mu and weights (all unequal) at a depth of two full batches
    and a remainder for that K: every layout and the uneven runs give the aligned single call's
    bits, which meet the reference.  K = 1 has w = 1: its radiances are path_radiance's bit for
    bit, on a vector and a scalar layout and across runs."""
    n = cases.angle_levels(angles)
    problem = cases.Problem(cases.ANGLE_COLUMNS, n, seed=300 + angles)
    sets = cases.run_sets(n)
    bands = small_bands(problem.columns)
    with Grid(engine, problem.nu) as grid:
        for name, run, expect in variants("flux", bands, angles):
            base = run(engine, grid, problem, "aligned", sets["whole"])
            check("flux", (angles, name), base, expect(problem, base))
            for layout in cases.LAYOUTS:
                for run_name in ("whole", "uneven", "uneven mirrored"):
                    got = run(engine, grid, problem, layout, sets[run_name])
                    assert_same(got, base, (angles, name, layout, run_name))
                    between = {k: v for k, v in got.items() if "@" in k}
                    rules = expect(problem, between)
                    check("flux", (angles, name, layout, run_name), between,
                          {k: rules[k] for k in between})
        if angles == 1:
            lengths, weight = problem.lengths(1)
            assert weight[0] == 1.
            slant = cases.Problem(cases.ANGLE_COLUMNS, n, seed=300 + angles)
            slant.thickness = lengths[:, 0]
            for layout in ("aligned", "odd"):
                for run_name in ("whole", "uneven", "uneven mirrored"):
                    for surface in ("first", "last"):
                        from_last = surface == "first"      # the down sweep
                        flux = run_flux(engine, grid, problem, layout, sets[run_name], 1, surface)
                        rad = run_radiance(engine, grid, slant, layout, sets[run_name],
                                           "cumulative", from_last, boundary=False)
                        what = (layout, run_name, surface)
                        assert same_bits(flux["down"], cases.FLUX_PI*(1.*rad["rad"])), what
                        final = cases._flat(n, 0 if from_last else n - 1)
                        assert same_bits(flux["reflection"], rad["rad"][final]), what
                        carried = [k for k in rad if "@" in k]
                        assert len(carried) == (0 if run_name == "whole" else 2)
                        for key in carried:
                            assert same_bits(flux["down " + key][0], rad[key]), (what, key)
    print("worst error / bound so far:", WORST)


@pytest.mark.parametrize("name,columns,bands", cases.BAND_SETS, ids=[x[0] for x in cases.BAND_SETS])
def test_band_segments(engine, name, columns, bands):
    """Segments of 1, 63, 64, 65 and 4096 columns, bands that end or start on a multiple of 4096,
    one over three segments, empty bands at 0, inside and at `columns` (NaN exactly), a band that
    ends at an odd `columns`: tau, exp(-tau), radiance and flux means, per path and per level;
    a second call gives the same bits."""
    problem = cases.Problem(columns, 3, seed=400 + columns)
    runs = cases.run_sets(3)["whole"]
    with Grid(engine, problem.nu) as grid:
        for kernel in ("path", "radiance", "flux"):
            for variant, run, expect in variants(kernel, bands):
                if "bands" not in variant:
                    continue
                got = run(engine, grid, problem, "aligned", runs)
                check(kernel, (kernel, name, variant), got, expect(problem, got))
                means = [k for k in got if k.endswith("mean")]
                assert means
                for key in means:
                    empty = np.diff(bands) == 0
                    assert np.all(np.isnan(got[key][:, empty])), key
                    assert not np.any(np.isnan(got[key][:, ~empty])), key
                assert_same(run(engine, grid, problem, "aligned", runs), got, "repeated")
                assert_same(run(engine, grid, problem, "exact", runs), got, "scalar")
    print("worst error / bound so far:", WORST)


def test_values_chosen_for_the_arithmetic(engine):
    """The extreme-value table of tests/sweep_cases.py (beta = 0, saturating layers, beta of mixed
    sign, nu = 0, Planck arguments that overflow expm1, boundaries so cold that the radiance
    underflows): NaN, inf and exact zeros fall where the float64 numpy loop has them (nowhere NaN
    or inf), numbers meet the long-double reference; on a vector and a scalar layout, whole and
    in uneven runs."""
    v = cases.value_problem()
    n, group = v.levels_per_path, v.group
    sets = cases.run_sets(n)
    with Grid(engine, v.nu) as grid:
        for kernel in ("path", "radiance", "flux"):
            for name, run, expect in variants(kernel):
                base = run(engine, grid, v, "aligned", sets["whole"])
                check(kernel, ("values", kernel, name), base, expect(v, base))
                for layout in ("aligned", "odd"):
                    for run_name in ("uneven", "uneven mirrored", "levels"):
                        assert_same(run(engine, grid, v, layout, sets[run_name]), base,
                                    (kernel, name, layout, run_name))
        for from_last in (False, True):
            last = cases._flat(n, 0 if from_last else n - 1)
            got = run_path(engine, v, "aligned", sets["whole"], "cumulative", from_last)
            loop, _ = cases.sweep_tau(F64, v.beta, v.thickness, n, from_last)
            with np.errstate(under="ignore"):
                assert cases.same_pattern(got["trans"], np.exp(-loop))
            assert np.all(got["tau"][:, group == 0] == 0.)
            assert np.all(got["trans"][:, group == 0] == 1.)
            assert np.all(got["trans"][last][:, group == 1] == 0.)

            start = cases.boundary_start(F64, v.nu, v.boundary_t, v.boundary_e)
            loop, _ = cases.sweep_radiance(F64, v.nu, v.beta, v.thickness, v.temperature, n,
                                           from_last, start)
            got = run_radiance(engine, grid, v, "aligned", sets["whole"], "cumulative", from_last)
            assert cases.same_pattern(got["rad"], loop)
            assert cases.same_pattern(got["bt"], cases.brightness(F64, v.nu, loop))
            # beta = 0: the boundary term at every level, the same bits from level to level (the
            # term itself meets the reference above; device expm1 is not numpy's to the bit)
            still = got["rad"][:, group == 0].reshape(PATHS, n, -1)
            assert same_bits(still, np.repeat(still[:, :1], n, axis=1))
            close("radiance", "boundary term", still[:, 0],
                  cases.boundary_start(LD, v.nu, v.boundary_t, v.boundary_e)[:, group == 0],
                  cases.boundary_start(LD, v.nu, v.boundary_t, v.boundary_e)[:, group == 0])
            saturated = cases.planck(LD, v.nu, v.temperature[last, None])[:, group == 1]
            close("radiance", "saturated", got["rad"][last][:, group == 1], saturated, saturated)
            assert np.all(got["rad"][:, 0] == 0.) and np.all(got["bt"][:, 0] == 0.)

            lengths, weight = v.lengths(3)
            down = cases.sweep_flux(F64, v.nu, v.beta, lengths, weight, v.temperature, n,
                                    from_last)
            begin, _ = cases.surface_start(F64, v.nu, v.surface_t, v.surface_e, down.total,
                                           down.total_mag)
            up = cases.sweep_flux(F64, v.nu, v.beta, lengths, weight, v.temperature, n,
                                  not from_last, begin)
            got = run_flux(engine, grid, v, "aligned", sets["whole"], 3,
                           "first" if from_last else "last")
            assert cases.same_pattern(got["down"], down.flux)
            assert cases.same_pattern(got["up"], up.flux)
            assert cases.same_pattern(got["reflection"], down.total)
            assert np.all(got["down"][:, 0] == 0.) and np.all(got["up"][:, 0] == 0.)
    print("worst error / bound so far:", WORST)
