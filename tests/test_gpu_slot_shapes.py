"""The cross-section and continuum slots (csrc/xsec.h, csrc/continuum.h, SlotCall::run of
csrc/slot_entry.inc) at the shapes their kernels branch on: every band size and band count of
tests/slot_cases.py on grids whose workgroup boundaries stand on knots, search windows of exactly
1023 / 1024 / 1025 frequencies, every last-workgroup shape on rows that are not 16-byte aligned,
grids in other orders, arithmetic grids cut against the coarse knots so that a wavefront's run is
of every class add_band tells apart, and calls of more than 65535 levels.
tests/test_slot_cases_host.py proves on the CPU that each case reaches the route it is named for.

Bounds are the project's contract and nothing tighter: assert_close of test_gpu_xsec.py (1e-6 of
the value plus 1e-12 of the spectrum maximum) and close of test_gpu_fuzz_slots.py.  On top of them
a point outside every band is exactly 0.0, and so is a point on a coarse knot whose table value is
0 (numpy.interp returns fp[j] itself on a knot).  Bit equality only where the project claims it:
a group against one call per continuum, chunks against rows of the same operands, a call repeated."""
import numpy as np
import pytest

from tests import slot_cases as cases
from tests.test_gpu_fuzz_slots import close
from tests.test_gpu_xsec import assert_close

pytestmark = pytest.mark.gpu

INSTANCES = list(cases.INSTANCES.values())
WORST = {}      # test group -> worst |got - oracle| / spectrum maximum


def note(group, got, expect):
    finite = np.isfinite(expect)
    scale = np.max(np.abs(expect[finite])) if finite.any() else 0.
    if scale > 0.:
        worst = float(np.max(np.abs(got[finite] - expect[finite]))/scale)
        WORST[group] = max(WORST.get(group, 0.), worst)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    yield default_engine(0)
    for group, worst in sorted(WORST.items()):
        print("\nworst difference from the oracle, %s: %.2e of the spectrum maximum" % (group, worst))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Block(object):
    """[rows, stride] float64 in HBM, pre-filled: a torch tensor behind DeviceSpectra's pointer /
    shape protocol (DeviceSpectra itself can only be written by the kernels under test)."""
    def __init__(self, engine, rows, stride, fill):
        import torch
        self.tensor = torch.full((rows, stride), fill, dtype=torch.float64, device="cuda:0")
        self.pointer, self.shape = self.tensor.data_ptr(), (rows, stride)
        assert self.pointer % 16 == 0
        engine.order_after_stream(torch.cuda.current_stream("cuda:0").cuda_stream)

    def host(self):
        return self.tensor.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# Cross-sections.
def xsec_expect(bands, grid, t, p):
    from oracle import xsec_oracle
    return np.stack([xsec_oracle.absorption_coefficient(bands, grid, t[i], p[i])
                     for i in range(len(t))])


def check_xsec(group, label, bands, grid, got, expect):
    for level in range(expect.shape[0]):
        assert_close(got[level], expect[level], f"{label}, level {level}")
    outside = cases.outside_every_band(bands, grid)
    assert np.all(expect[:, outside] == 0.) and np.all(got[:, outside] == 0.), label
    assert np.array_equal(got[:, outside] == 0., expect[:, outside] == 0.), label
    note(group, got, expect)


def run_xsec(engine, handle, grid, count):
    t, p = cases.levels(count)
    grid_handle = engine.load_grid(grid)
    try:
        return np.array(engine.xsec_compute(handle, grid_handle, grid.size, t, p)), t, p
    finally:
        engine.free_grid(grid_handle)


@pytest.mark.parametrize("count", cases.COUNTS)
@pytest.mark.parametrize("size", cases.SIZES)
def test_xsec_band_sizes_and_counts(engine, size, count):
    """Every band size x band count on the knots grid and the edges grid, with 1 level (<4,1>)
    and 5 (<2,4>, a partial level group); 2, 3, 4, 8 and 9 levels on one case."""
    bands = cases.molecule(size, count)
    handle = engine.load_xsec(bands)
    counts = (1, 5) + (cases.LEVEL_COUNTS if (size, count) == (129, 3) else ())
    try:
        for name, grid in (("knots", cases.knots_grid(bands)), ("edges", cases.edges_grid(bands)[0])):
            for n_levels in counts:
                got, t, p = run_xsec(engine, handle, grid, n_levels)
                check_xsec("xsec sizes and counts", f"{size} x {count} on {name}, {n_levels} level(s)",
                           bands, grid, got, xsec_expect(bands, grid, t, p))
    finally:
        engine.free_xsec(handle)


@pytest.mark.parametrize("from_start", (False, True))
@pytest.mark.parametrize("length", cases.WINDOWS)
@pytest.mark.parametrize("instance", INSTANCES, ids=lambda i: i.name)
def test_xsec_window_sizes(engine, instance, length, from_start):
    """The first workgroup's staged range is exactly `length` frequencies: in LDS up to 1024, in
    HBM from 1025; from_start: the window begins at the band's first frequency."""
    band = cases.window_band()
    grid = cases.window_grid(band, length, instance, from_start)
    handle = engine.load_xsec([band])
    try:
        got, t, p = run_xsec(engine, handle, grid, instance.levels)
        again, _, _ = run_xsec(engine, handle, grid, instance.levels)
    finally:
        engine.free_xsec(handle)
    check_xsec("xsec window sizes", f"window {length}", [band], grid, got,
               xsec_expect([band], grid, t, p))
    assert same_bits(got, again)


@pytest.mark.parametrize("n", cases.TAILS)
@pytest.mark.parametrize("instance", INSTANCES, ids=lambda i: i.name)
def test_xsec_tails_on_odd_strides(engine, instance, n):
    """Last-workgroup shapes and pair tails on a block in HBM whose odd row stride leaves every
    second row off 16-byte alignment: a write leaves no NaN of the pre-fill in the first n
    columns, an accumulate adds onto a known value, the padding keeps its bits in both."""
    bands = cases.molecule(129, 3)
    grid = cases.tail_grid(bands, n)
    stride = n + 1 + n % 2
    assert stride % 2 == 1
    t, p = cases.levels(instance.levels)
    expect = xsec_expect(bands, grid, t, p)
    handle, grid_handle = engine.load_xsec(bands), engine.load_grid(grid)
    try:
        for fill, accumulate in ((np.nan, False), (3.e-23, True)):
            block = Block(engine, instance.levels, stride, fill)
            before = block.host()
            engine.xsec_compute(handle, grid_handle, n, t, p, out=block, accumulate=accumulate)
            after = block.host()
            assert same_bits(after[:, n:], before[:, n:]), "the padding was written"
            got = after[:, :n]
            assert not np.isnan(got).any()
            wanted = expect + fill if accumulate else expect
            for level in range(instance.levels):
                assert_close(got[level], wanted[level], f"{n} points, accumulate={accumulate}")
            outside = cases.outside_every_band(bands, grid)
            assert np.all(got[:, outside] == (fill if accumulate else 0.))
            note("xsec tails", got, wanted)
    finally:
        engine.free_grid(grid_handle)
        engine.free_xsec(handle)


@pytest.mark.parametrize("instance", INSTANCES, ids=lambda i: i.name)
def test_xsec_grids_in_other_orders(engine, instance):
    """Descending, shuffled (the branch that takes whole bands as windows), repeated neighbours,
    0 and negative wavenumbers, grids wholly below and above the bands."""
    bands = cases.molecule(129, 3)
    grids, permutation = cases.order_grids(bands)
    handle = engine.load_xsec(bands)
    got = {}
    try:
        for name, grid in grids.items():
            got[name], t, p = run_xsec(engine, handle, grid, instance.levels)
            check_xsec("xsec grid orders", name, bands, grid, got[name],
                       xsec_expect(bands, grid, t, p))
    finally:
        engine.free_xsec(handle)
    for level in range(instance.levels):
        assert_close(got["shuffled"][level], got["ascending"][level][permutation], "shuffled")
        assert_close(got["descending"][level], got["ascending"][level][::-1], "descending")
    assert not got["below every band"].any() and not got["above every band"].any()


def test_xsec_bands_at_model_sizes(engine):
    """xsec_model_kernel strides a band over 1024 threads: 2, 1023, 1024, 1025 and 4097
    frequencies, a band whose fit sums negative (clipped, not rescaled) and one without a negative
    value, against full_model with the same points clipped."""
    from oracle import xsec_oracle
    bands = cases.model_bands()
    handle = engine.load_xsec(bands)
    try:
        for t, p in zip(*cases.levels(3)):
            got = engine.xsec_bands(handle, [b[0].size for b in bands], t, p)
            for k, (_, coefficients) in enumerate(bands):
                expect = xsec_oracle.full_model(t, p, coefficients)
                assert_close(got[k], expect, f"band {k} of {coefficients.shape[1]}")
                assert np.array_equal(got[k] == 0., expect == 0.), k
                note("xsec fit model", got[k], expect)
    finally:
        engine.free_xsec(handle)


# ---------------------------------------------------------------------------------------------
# Continua.
@pytest.fixture(scope="module")
def continua():
    from pylbl_amd import mt_ckd
    return {owner: mt_ckd.CONTINUA[owner]() for owner in cases.OWNERS}


def atmosphere(count):
    from pylbl_amd import synthetic
    atmos = synthetic.standard_atmosphere(max(count, 2))
    return atmos.t[:count], atmos.p[:count], {k: v[:count] for k, v in atmos.vmr.items()}


def continuum_expect(continuum_oracle, owner, t, p, vmr, grid):
    return np.stack([continuum_oracle.continuum(owner).spectra(
        t[i], p[i], {k: v[i] for k, v in vmr.items()}, grid) for i in range(len(t))])


def exact_zeros(continuum_oracle, owner, grid):
    """Points outside every band of the continuum, and points bit-equal to a coarse knot."""
    outside, knot = np.ones(grid.size, dtype=bool), np.zeros(grid.size, dtype=bool)
    for w, _, _ in continuum_oracle.continuum(owner).bands:
        outside &= (grid < w[0]) | (grid > w[-1])
        knot |= np.isin(grid, w)
    return outside, knot


RUN_GRIDS = ("low aligned", "low ending on knots", "low knots inside", "low between knots",
             "high ending on knots", "high knots inside", "high aligned", "descending", "linspace",
             "short")


@pytest.mark.parametrize("name", RUN_GRIDS)
@pytest.mark.parametrize("instance", INSTANCES, ids=lambda i: i.name)
@pytest.mark.parametrize("owner", cases.OWNERS)
def test_continuum_run_classes(engine, continua, continuum_oracle, owner, instance, name):
    """The grid `name` of slot_cases.run_grids cut for the runs of `instance` against the first
    band of `owner`: one continuum with 1 and 5 levels (<4,1>, <2,4>) against the oracle, the
    groups (H2OForeign, H2OSelf) and all six through continuum_compute_many (<4,1>, <4,2>), writing
    and adding, bit for bit against one call per continuum and against the oracle's sum."""
    from pylbl_amd import mt_ckd
    from pylbl_amd.engine import DeviceSpectra
    knots = continuum_oracle.continuum(owner).bands[cases.TARGET_BAND][0]
    grid = np.ascontiguousarray(cases.run_grids(cases.coarse_of(knots), instance)[name])
    assert list(cases.run_grids(cases.coarse_of(knots), instance)) == list(RUN_GRIDS)
    for count in (1, 5):
        t, p, vmr = atmosphere(count)
        expect = {o: continuum_expect(continuum_oracle, o, t, p, vmr, grid) for o in cases.OWNERS}
        got = np.array(continua[owner].spectra_levels(t, p, vmr, grid))
        close(got, expect[owner], f"{owner} on {name}, {count} level(s)")
        outside, knot = exact_zeros(continuum_oracle, owner, grid)
        assert np.all(expect[owner][:, outside] == 0.) and np.all(got[:, outside] == 0.)
        on_zero_knot = knot[None, :] & (expect[owner] == 0.)
        assert np.all(got[on_zero_knot] == 0.), f"{owner} on {name}: a knot whose value is 0"
        assert same_bits(got, np.array(continua[owner].spectra_levels(t, p, vmr, grid)))
        note("one continuum", got, expect[owner])
        for owners in cases.GROUPS:
            members = [continua[o] for o in owners]
            for adding in (False, True):
                padded = grid.size + 9
                one_by_one = DeviceSpectra(engine, count, padded)
                together = DeviceSpectra(engine, count, padded)
                try:
                    if adding:
                        for block in (one_by_one, together):
                            continua["O3"].spectra_levels(t, p, vmr, grid, out=block)
                    for i, continuum in enumerate(members):
                        continuum.spectra_levels(t, p, vmr, grid, out=one_by_one,
                                                 accumulate=adding or i > 0, asynchronous=True)
                    mt_ckd.spectra_levels_many(members, t, p, vmr, grid, together,
                                               accumulate=adding, asynchronous=True)
                    engine.synchronize()
                    a = one_by_one.to_host()[:, :grid.size]
                    b = together.to_host()[:, :grid.size]
                finally:
                    one_by_one.free()
                    together.free()
                assert same_bits(a, b), (owners, name, count, adding)
                total = sum(expect[o] for o in owners) + (expect["O3"] if adding else 0.)
                close(b, total, f"group {owners} on {name}, adding={adding}", floor=1e-12)
                note("groups of continua", b, total)


# ---------------------------------------------------------------------------------------------
# More than 65535 levels: the second chunk of SlotCall::run.
MANY = 65539


def check_rows(got, expect, period, compare):
    compare(got[:period], expect)
    first = np.ascontiguousarray(got[:period]).view(np.uint64)
    rows = np.ascontiguousarray(got).view(np.uint64)
    wrong = np.flatnonzero(np.any(rows != first[np.arange(got.shape[0]) % period], axis=1))
    assert wrong.size == 0, f"rows {wrong[:8]} differ from the rows of the same operands"


def test_xsec_more_than_65535_levels(engine):
    """65539 levels into a block in HBM: 65535 in the first chunk, 4 in the second.  (T, p, vmr)
    repeat with period 7: rows 0..6 against the oracle, every row bit for bit against row r % 7."""
    from pylbl_amd import number_density
    from pylbl_amd.engine import DeviceSpectra
    bands = [cases.xsec_band(2, 700., 31), cases.xsec_band(3, 700.02, 32)]
    w = cases.band_wavenumbers(bands[1])
    grid = np.asarray([699.99, w[0], 0.5*(w[0] + w[1]), w[2], w[2] + 1.])
    t, p = cases.levels(MANY, 7)
    vmr = 1e-10*(1. + np.arange(MANY) % 7)
    expect = number_density(t[:7], p[:7], vmr[:7])[:, None]*xsec_expect(bands, grid, t[:7], p[:7])
    handle, grid_handle = engine.load_xsec(bands), engine.load_grid(grid)
    block = DeviceSpectra(engine, MANY, 10)
    try:
        engine.xsec_compute(handle, grid_handle, grid.size, t, p, vmr=vmr, out=block)
        got = block.to_host()[:, :grid.size]
    finally:
        block.free()
        engine.free_grid(grid_handle)
        engine.free_xsec(handle)

    def compare(rows, reference):
        for level in range(7):
            assert_close(rows[level], reference[level], f"level {level}")
        assert not rows[:, 0].any() and not rows[:, -1].any() and rows[:, 2].all()
        note("65539 levels", rows, reference)
    check_rows(got, expect, 7, compare)


def test_continuum_more_than_65535_levels(engine, continua, continuum_oracle):
    """The same for a shipped continuum: N2, the one with the fewest coarse points (492: its
    spectra and slopes of a 65535-level chunk take 516 MB)."""
    from pylbl_amd.engine import DeviceSpectra
    sizes = {o: sum(w.size for w, _, _ in continuum_oracle.continuum(o).bands) for o in cases.OWNERS}
    assert min(sizes, key=sizes.get) == "N2" and 2*8*65535*sizes["N2"] < 1 << 30
    t7, p7, vmr7 = atmosphere(7)
    index = np.arange(MANY) % 7
    t, p, vmr = t7[index], p7[index], {k: np.ascontiguousarray(v[index]) for k, v in vmr7.items()}
    grid = np.asarray([-15., 0., 2.5, 2200., 4500.])
    expect = continuum_expect(continuum_oracle, "N2", t7, p7, vmr7, grid)
    block = DeviceSpectra(engine, MANY, 10)
    try:
        continua["N2"].spectra_levels(t, p, vmr, grid, out=block)
        got = block.to_host()[:, :grid.size]
    finally:
        block.free()

    def compare(rows, reference):
        close(rows, reference, "N2, rows 0..6")
        assert not rows[:, :2].any() and rows[:, 2:].all()
        note("65539 levels", rows, reference)
    check_rows(got, expect, 7, compare)


def test_group_of_65536_levels(engine, continua, continuum_oracle):
    """The group call cuts its levels into runs of 65535 like SlotCall::run (it refused them
    once): 65536 levels, the second run one level (group_interp_kernel<4, 1>), rows 0..6 against
    the oracle and every row bit for bit against row r % 7; then the same group on seven levels."""
    from pylbl_amd import mt_ckd
    from pylbl_amd.engine import DeviceSpectra
    grid = np.asarray([-15., 0., 2.5, 2200., 4500.])
    members = [continua["H2OForeign"], continua["H2OSelf"]]
    t7, p7, vmr7 = atmosphere(7)
    index = np.arange(65536) % 7
    block = DeviceSpectra(engine, 65536, grid.size)
    try:
        mt_ckd.spectra_levels_many(members, t7[index], p7[index],
                                   {k: np.ascontiguousarray(v[index]) for k, v in vmr7.items()},
                                   grid, block)
        many = block.to_host()
        rows = block.rows(7)
        mt_ckd.spectra_levels_many(members, t7, p7, vmr7, grid, rows)
        got = rows.to_host()
    finally:
        block.free()
    expect = sum(continuum_expect(continuum_oracle, o, t7, p7, vmr7, grid)
                 for o in ("H2OForeign", "H2OSelf"))
    close(got, expect, "the group on seven levels", floor=1e-12)
    assert same_bits(many[:7], got)
    check_rows(many, expect, 7, lambda rows, reference: close(rows, reference, "rows 0..6",
                                                              floor=1e-12))
