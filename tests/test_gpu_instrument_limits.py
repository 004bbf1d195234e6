"""lbl_instrument_apply fed directly (Engine.instrument_create / instrument_apply on rows held in
torch tensors) at the shapes where a rewrite of instrument.h breaks first: the identity probe
(every window column by column, at tile and segment edges, on a uniform and a non-uniform grid),
row groups and row offsets, more rows than a launch grid's y dimension, the partial-sum cap that
splits rows into launches, NaN outside the windows, the NaN rules at their edges, state left by
earlier calls, and Spectroscopy rows over several row groups.  The reference sums in extended
precision (tests/instrument_cases.py); the tolerance is the suite's 1e-12 * sum|w v| / |sum w|."""
import contextlib

import numpy as np
import pytest

from pylbl_amd import Instrument
from tests import instrument_cases as cases

pytestmark = pytest.mark.gpu

# |w| below this may differ from numpy's by a few ulps of 1 next to a zero of a sinc (device
# sin / exp against numpy's): the absolute allowance of the Gaussian and FTS shapes, over sum w.
ALLOWANCE = 4.*2.**-53
LIBM_SHAPES = ("gaussian", "fts", "fts-hamming")
SENTINEL = -12345.678


class Rows(object):
    """A float64 torch tensor [rows, row stride] on the GPU, as the engine's values or out."""
    def __init__(self, tensor):
        assert tensor.dtype.is_floating_point and tensor.stride(1) == 1
        self.tensor = tensor
        self.pointer, self.shape = tensor.data_ptr(), tuple(tensor.shape)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def device_rows(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float64)).to("cuda:0")


@contextlib.contextmanager
def bound(engine, instrument, grid):
    """The handle of `instrument` on a grid of its own, freed afterwards."""
    grid_handle = engine.load_grid(grid)
    handle = instrument._create(engine, grid_handle)        # Engine.instrument_create
    try:
        yield handle
    finally:
        engine.synchronize()
        engine.instrument_free(handle)
        engine.free_grid(grid_handle)


def apply(engine, handle, values, rows, channels, transmittance=False, out=None,
          asynchronous=False):
    """Channels of the first `rows` rows of the tensor `values`: [rows, channels] on the host."""
    import torch
    if out is None:
        out = torch.full((rows, channels), SENTINEL, dtype=torch.float64, device=values.device)
    engine.order_after_stream(torch.cuda.current_stream(values.device).cuda_stream)
    engine.instrument_apply(Rows(values), rows, handle, Rows(out), transmittance=transmittance,
                            asynchronous=asynchronous)
    engine.synchronize()
    return out[:rows].cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check(got, instrument, grid, rows):
    mean, error, _ = cases.reference(instrument, grid, rows)
    got = np.asarray(got).reshape(mean.shape)
    assert np.array_equal(np.isnan(got), np.isnan(mean))
    ok = ~np.isnan(mean)
    worst = np.max(np.abs(got[ok] - mean[ok]) - error[ok], initial=-1.)
    assert np.all(np.abs(got[ok] - mean[ok]) <= error[ok] + 1e-300), worst


def scaled_rows(bases, rows):
    """Row r = bases[r % len(bases)] * 2^(r % 11 - 5) on the GPU, and the scales."""
    import torch
    r = np.arange(rows)
    scale = np.ldexp(1., r % 11 - 5)
    index = torch.from_numpy(r % len(bases)).to("cuda:0")
    values = device_rows(bases)[index]
    values *= device_rows(scale)[:, None]
    return values, r % len(bases), scale


@pytest.mark.parametrize("kind", ["uniform", "jittered"])
@pytest.mark.parametrize("name", cases.SHAPE_NAMES)
def test_identity_probe_is_the_normalised_response(engine, kind, name):
    """Row j = e_j: channel c of row j is w_c(nu_j)/sum w_c, exactly 0 outside the window and
    non-zero exactly where w_c(nu_j) is, whatever its size; with transmittance and +inf at column
    j, (sum w - w_j)/sum w.  A column dropped or added at a window's, segment's or tile's edge
    fails here."""
    import torch
    grid = cases.probe_grid(kind)
    x = cases.probe_instrument(name, grid)
    m, n = grid.size, len(x)
    eye = torch.eye(m, dtype=torch.float64, device="cuda:0")
    with bound(engine, x, grid) as handle:
        got = apply(engine, handle, eye, m, n)
        infinite = torch.where(eye > 0., torch.full_like(eye, np.inf), torch.zeros_like(eye))
        del eye
        through = apply(engine, handle, infinite, m, n, transmittance=True)
        del infinite
    start, end = x.columns(grid)
    covered = x.covered(grid)
    libm = name in LIBM_SHAPES
    for c in range(n):
        w = cases.channel_weights(x, grid, c) if covered[c] else None
        if w is None or not w.sum() > 0.:
            assert np.all(np.isnan(got[:, c])) and np.all(np.isnan(through[:, c])), c
            continue
        s, e = start[c], end[c]
        total = np.sum(w.astype(np.longdouble))
        allowance = ALLOWANCE/abs(float(total)) if libm else 0.
        column = got[:, c]
        assert np.all(column[:s] == 0.) and np.all(column[e:] == 0.), c
        exact = np.abs(w) > ALLOWANCE if libm else np.ones(w.size, dtype=bool)
        assert np.array_equal((column[s:e] != 0.)[exact], (w != 0.)[exact]), c
        expect = (w.astype(np.longdouble)/total).astype(np.float64)
        assert np.all(np.abs(column[s:e] - expect) <=
                      1e-12*np.abs(w)/abs(float(total)) + allowance), c
        # exp(-inf) = 0 at column j, exp(-0) = 1 elsewhere
        expect = np.ones(m)
        expect[s:e] = ((total - w.astype(np.longdouble))/total).astype(np.float64)
        error = np.full(m, 1e-12*np.sum(np.abs(w))/abs(float(total)))
        error[s:e] -= 1e-12*np.abs(w)/abs(float(total))
        assert np.all(np.abs(through[:, c] - expect) <= error + allowance), c
    # duplicated channels: the same bits
    lo, hi = x.window()
    for a in range(n):
        for b in range(a + 1, n):
            if covered[a] and lo[a] == lo[b] and hi[a] == hi[b]:
                assert same_bits(got[:, a], got[:, b]) and same_bits(through[:, a], through[:, b])


def test_row_groups_and_row_offsets(engine):
    """1 to 200 rows (partial row stagings of 8, whole and partial row groups of 64) give the
    bits of the same rows of one 205-row call, from row 0 and from row 5 (a sliced pointer);
    signed values of magnitudes 1e-150 to 1e150 on a non-uniform grid."""
    grid = cases.probe_grid("jittered")
    x = cases.probe_instrument("gaussian", grid)
    rng = np.random.default_rng(21)
    total = 205
    values = rng.choice([-1., 1.], (total, grid.size))*10.**rng.uniform(-150., 150.,
                                                                        (total, grid.size))
    rows = device_rows(values)
    with bound(engine, x, grid) as handle:
        whole = apply(engine, handle, rows, total, len(x))
        check(whole, x, grid, values)
        for count in (1, 7, 8, 9, 63, 64, 65, 200):
            assert same_bits(apply(engine, handle, rows, count, len(x)), whole[:count]), count
            assert same_bits(apply(engine, handle, rows[5:], count, len(x)),
                             whole[5:5 + count]), count


def test_more_rows_than_the_launch_grid_y_dimension(engine):
    """65 535 + 77 rows: two launches.  Row r is a base row times 2^(r % 11 - 5), so its channels
    are the base row's times that power, bit for bit."""
    grid = cases.probe_grid("jittered", size=1003)
    x = Instrument.gaussian(np.arange(600.5, 615.4, 0.35), 0.4, half_width=1.2)
    rows = cases.GRID_Y + 77
    tiles = cases.tiling(x, grid)
    assert cases.launch_chunk(len(tiles["items"]), rows) == cases.GRID_Y
    rng = np.random.default_rng(22)
    bases = rng.uniform(-1., 1., (3, grid.size))*10.**rng.uniform(-3., 3., (3, grid.size))
    values, base_of, scale = scaled_rows(bases, rows)
    with bound(engine, x, grid) as handle:
        base = apply(engine, handle, device_rows(bases), 3, len(x))
        check(base, x, grid, bases)
        got = apply(engine, handle, values, rows, len(x))
    del values
    assert np.array_equal(got, base[base_of]*scale[:, None], equal_nan=True)


def test_the_partial_sum_cap_splits_rows(engine):
    """64 channels whose windows span a grid of 2^20 points: 8192 items, so that 2^24 partials
    hold 64 rows, and 150 rows take three launches."""
    m = 1 << 20
    grid = 600. + np.arange(m)/1024.
    i = np.arange(64)
    lo, hi = grid[i], grid[m - 1 - i]
    x = Instrument.triangle((lo + hi)/2., (hi - lo)/2.)
    tiles = cases.tiling(x, grid)
    assert len(tiles["items"]) == 8192
    rows = 150
    chunk = cases.launch_chunk(len(tiles["items"]), rows)
    assert chunk == 64 < rows
    rng = np.random.default_rng(23)
    bases = rng.uniform(-1., 1., (2, m))*10.**rng.uniform(-3., 3., (2, m))
    values, base_of, scale = scaled_rows(bases, rows)
    with bound(engine, x, grid) as handle:
        base = apply(engine, handle, device_rows(bases), 2, len(x))
        got = apply(engine, handle, values, rows, len(x))
    del values
    check(base, x, grid, bases)
    assert np.array_equal(got, base[base_of]*scale[:, None], equal_nan=True)


@pytest.mark.parametrize("name", ["gaussian", "triangle"])
def test_nothing_leaks_in_from_outside_the_windows(engine, name):
    """Rows longer than the grid, spare rows, and every column no valid window covers hold NaN;
    out rows past `rows` hold a sentinel.  The channels are the bits of the call on clean rows,
    plain and through exp(-v), and the sentinel rows are untouched."""
    import torch
    grid = cases.probe_grid("jittered")
    x = cases.probe_instrument(name, grid)
    m, n, rows = grid.size, len(x), 70
    tiles = cases.tiling(x, grid)
    inside = np.zeros(m, dtype=bool)
    for c in np.flatnonzero(tiles["valid"]):
        inside[tiles["begin"][c]:tiles["end"][c]] = True
    assert not np.all(inside)
    clean = np.random.default_rng(24).uniform(0.1, 3., (rows, m))
    dirty = np.full((rows + 3, m + 37), np.nan)
    dirty[:rows, :m] = np.where(inside, clean, np.nan)
    clean_rows, dirty_rows = device_rows(clean), device_rows(dirty)
    with bound(engine, x, grid) as handle:
        for transmittance in (False, True):
            expect = apply(engine, handle, clean_rows, rows, n, transmittance=transmittance)
            if not transmittance:
                check(expect, x, grid, clean)
            else:
                check(expect, x, grid, np.exp(-clean))
            out = torch.full((rows + 5, n), SENTINEL, dtype=torch.float64, device="cuda:0")
            apply(engine, handle, dirty_rows, rows, n, transmittance=transmittance, out=out)
            got = out.cpu().numpy()
            assert same_bits(got[:rows], expect)
            assert np.all(got[rows:] == SENTINEL)


def test_nan_rules_at_their_edges(engine):
    """Weights that sum to exactly 0 (a triangle whose only points lie at +/- fwhm), that
    underflow to 0 (a very narrow Gaussian), that sum to < 0 (a table), and an instrument with
    no valid channel at all (no items) on 70 rows: NaN exactly where numpy says so."""
    grid = cases.probe_grid("uniform")
    step = cases.STEP
    edge = grid[100] + step/2.
    triangle = Instrument.triangle([edge, grid[300], grid[700] + step/4.], [step/2., 0.5, 0.3])
    start, end = triangle.columns(grid)
    assert end[0] - start[0] == 2 and triangle.response(grid)[0].sum() == 0.
    narrow = Instrument.gaussian([edge, grid[400]], [1e-10, 0.3], half_width=[2.*step, 0.9])
    assert narrow.response(grid)[0].sum() == 0. and narrow.covered(grid)[0]
    table = Instrument.tabulated([grid[500], grid[900], grid[1300]], [-1., 0.3, 1.],
                                 [[-1., 0.5, 0.], [0.2, 1., 0.5], [0., -0.1, 0.]])
    assert table.response(grid)[0].sum() < 0. and table.response(grid)[2].sum() < 0.
    nothing = Instrument.boxcar([grid[0], grid[-1], grid[50] + step/4.], [1., 1., step/8.])
    assert not np.any(nothing.covered(grid)) and len(cases.tiling(nothing, grid)["items"]) == 0
    values = np.random.default_rng(25).uniform(0.5, 2., (70, grid.size))
    rows = device_rows(values)
    for x, count in ((triangle, 5), (narrow, 5), (table, 5), (nothing, 70)):
        with bound(engine, x, grid) as handle:
            got = apply(engine, handle, rows, count, len(x))
        numpy = x.apply(grid, values[:count])
        assert np.array_equal(np.isnan(got), np.isnan(numpy)), x
        check(got, x, grid, values[:count])
    assert np.isnan(got).all()


def test_state_from_earlier_calls(engine):
    """A small instrument after a large one on the same engine gives the bits of a fresh engine
    (nothing stale in the shared partial sums); asynchronous=True then synchronize() gives the
    bits of the synchronous call."""
    from pylbl_amd.engine import Engine
    grid = cases.probe_grid("jittered")
    large = cases.probe_instrument("fts", grid)
    small = Instrument.boxcar([602., 610.5, 630.], [0.5, 3., 1.])
    values = np.random.default_rng(26).uniform(-1., 2., (130, grid.size))
    rows = device_rows(values)
    with bound(engine, large, grid) as handle:
        apply(engine, handle, rows, 130, len(large))
    with bound(engine, small, grid) as handle:
        after = apply(engine, handle, rows, 130, len(small))
        later = apply(engine, handle, rows, 130, len(small), asynchronous=True)
    check(after, small, grid, values)
    assert same_bits(later, after)
    fresh = Engine(0)
    try:
        with bound(fresh, small, grid) as handle:
            assert same_bits(apply(fresh, handle, rows, 130, len(small)), after)
    finally:
        fresh.close()


def test_apply_refuses_an_out_of_the_wrong_width(engine):
    """out[r] starts at out + r*channels: an `out` of another width is refused before any
    launch."""
    import torch
    grid = cases.probe_grid("uniform")
    x = Instrument.boxcar([602., 605., 610.], 1.)
    rows = device_rows(np.zeros((2, grid.size)))
    with bound(engine, x, grid) as handle:
        for width in (2, 4):
            out = torch.zeros((2, width), dtype=torch.float64, device="cuda:0")
            with pytest.raises(ValueError, match="channels"):
                engine.instrument_apply(Rows(rows), 2, handle, Rows(out))
        engine.synchronize()


def test_spectroscopy_rows_over_several_row_groups():
    """compute_path with 150 paths and compute_radiance(cumulative=True) with 450 levels: three
    and eight row groups, in one run of levels and in several."""
    from tests.test_gpu_instrument import check as check_channels, lengths, spectroscopy
    shape = (150, 3)
    grid = np.arange(600., 620., 0.01)
    x = Instrument.gaussian(np.arange(601., 619.1, 0.25), 0.5, half_width=1.5)
    s = lengths(shape, seed=7)
    spec = spectroscopy(shape=shape, grid=grid)
    fine = spec.compute_path(s)
    got = spec.compute_path(s, instrument=x)
    assert np.asarray(got["optical_depth"]).shape == (150, len(x))
    for q in ("optical_depth", "transmittance"):
        check_channels(got[q], x, grid, fine[q])
    fine = spec.compute_radiance(s, boundary_temperature=290., cumulative=True)["radiance"]
    radiance = spec.compute_radiance(s, boundary_temperature=290., cumulative=True,
                                     instrument=x)["radiance"]
    assert np.asarray(radiance).size == 450*len(x)
    check_channels(radiance, x, grid, fine)
    split = spectroscopy(shape=shape, grid=grid)
    split.device_output_limit = 2*100*grid.size*8
    runs = split.compute_radiance(s, boundary_temperature=290., cumulative=True, instrument=x)
    np.testing.assert_array_equal(np.asarray(runs["radiance"]), np.asarray(radiance))
    paths = split.compute_path(s, instrument=x)
    for q in ("optical_depth", "transmittance"):
        np.testing.assert_array_equal(np.asarray(paths[q]), np.asarray(got[q]))
