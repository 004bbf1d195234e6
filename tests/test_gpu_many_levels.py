"""The lines call (lbl_compute: csrc/compute_call.inc, csrc/compute_stages.inc) past 65 535 levels
and on the largest grid it takes, and compute_absorption past 65 535 levels.  Inputs and their
mirrors: tests/many_levels_cases.py; tests/test_many_levels_cases_host.py proves on the CPU that each
case is what it is taken for here, and that with workspace_bytes = 64 GiB the 65535 in
levels_per_pass's min() is what cuts the passes of the big calls.

Part 1.  Calls of 65 535 (one full pass: gridDim.y == 65535 for every kernel of the pass), 65 536
(a second pass of one level, whose scalars travel inline), 65 547 (a second pass through the pinned
block) and 131 073 levels (three passes) repeat seven pattern levels.  Row l of a big call equals
row l % 7 of the same engine's seven-level call with the same options bit for bit ("results must
not depend on the chunking", tests/test_gpu_api.py); the seven-level call meets
oracle.absorption_port under tests.test_gpu_parity.assert_spectrum with its REL; rows past the call
and the padding of a strided block keep their sentinel; with LBL_ACCUMULATE a row is what was there
plus the row; `evals` is the seven-level counts multiplied out; a second call gives the same bits
and nothing is NaN.  The relaxation (scan_chain = 1) is held to bit equality on the level counts
whose every pass holds all seven pattern levels (relax_launches follows the pass's max_runs); on
the others (a pass of one or three levels) it is held to the oracle and to the serial chain within
the 1e-7 of the plain spectrum of tests/test_gpu_pedestal_many_runs.py.

Part 2 (test_largest_grid*).  One level on 1 073 709 056 points: zero outside every window (on the
device), every cluster of lines against a float64 sum of oracle.voigt_port over the lines whose
windows reach it, with four and with eight points per lane (the project claims no equality of bits
between tilings: each is held to the oracle), the far-field series, the pedestal's per-cell
structure, and the refusal one cell further.

Part 3.  Spectroscopy.compute_absorption on 65 538 levels (two gases with lines, the two banded
continua of H2O -- the group call --, one cross-section) against the same Spectroscopy on the seven
pattern levels, and lbl_continuum_compute_many on 65 537 levels against one call per continuum.
Before this file the group call refused more than 65 535 levels; it now cuts them into runs of
65 535 as SlotCall::run does for the one-slot calls.

Findings.  (1) lbl_continuum_compute_many refused more than 65 535 levels, so
compute_absorption raised on such an atmosphere as soon as a gas carried two banded continua
(test_compute_absorption_of_65538_levels; tests/test_gpu_slot_shapes.py held the refusal itself).
(2) prepare_line and inner_index_range (csrc/line_prep.h) clamped a line's core and inner index
ranges to 1e9, below the 2^30 - 1 points shape_of takes: on the largest grid the lines of the last
cluster, past index 1e9, lost their core rows and inner points -- relative error 8.3 in
test_largest_grid, where the four clusters below 1e9 stood at 1e-13.  The ceiling is 2^30 now.

What a wrong index costs: each change below was built once from a scratch copy of the sources and
this file run on it (none is in the tree; all are wrong-result changes, none faulted).
  * the 65535 taken out of levels_per_pass: test_passes_are_the_caps fails ((1, 1) launches for
    65 536 levels instead of (2, 2)) and nothing else does -- this runtime takes gridDim.y =
    131 073, and the kernels read blockIdx.y as it comes: the cap guards a launch limit, the
    results do not depend on it.
  * `base` dropped from rq.temperature[base + l]: every test of Part 1 fails but test_evals (the
    rows of the later passes are those of other temperatures; the window counts do not depend on
    T) -- and test_passes_are_the_caps, which counts launches, was written later and not run on it.
  * `base*c.shape.stride` dropped from pass_of: test_block_in_hbm_with_padded_rows (all three),
    test_accumulate (both) and test_streamed_call_in_pieces (both) fail -- every test with a block
    in HBM; the host-output tests pass.
  * `blockIdx.y & 0x7fff` in pedestal_apply_kernel: test_pedestal_serial_chain (both),
    test_pedestal_relaxation (both) and the pedestal cases of test_block_in_hbm_with_padded_rows,
    test_accumulate and test_streamed_call_in_pieces fail; the tests without a pedestal pass.

Wall time on an MI355X: 19 s for the file, of which 12 s are the first test that brings up torch
(test_block_in_hbm_with_padded_rows[small-False]) and its allocator.  test_largest_grid: 2.3 s
within the file, 13.1 s measured alone with torch's start in it -- the four calls take 0.31, 0.12,
0.15 and 0.01 s (plan_for's loop over 4.2 M tiles is in the first; the plans are kept), the float64
reference 0.35 s, the rest is five 19 MB slices per call over the host link.  Every other test
takes under 1.5 s (test_evals[1], host prologue: 1.0 s; the compute_absorption cases 0.4 - 0.7 s)."""
from ctypes import c_int64, c_void_p
import time

import numpy as np
import pytest

from tests import golden_io
from tests import many_levels_cases as cases
from tests.test_gpu_parity import assert_spectrum
from tests.test_gpu_pedestal_workspace import _options

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    e.set_option("workspace_bytes", cases.WORKSPACE)
    handles = {}

    def handle(name):
        if name not in handles:
            handles[name] = e.load(cases.table(name))
        return handles[name]
    e.handle_of = handle
    yield e
    _options(e, 1, 0, 0)
    e.close()


class Block(object):
    """[rows, stride] float64 in HBM, pre-filled with a value or an array: a torch tensor behind
    DeviceSpectra's pointer / shape protocol."""
    def __init__(self, rows, stride, fill):
        import torch
        if np.ndim(fill) == 0:
            self.tensor = torch.full((rows, stride), float(fill), dtype=torch.float64,
                                     device="cuda:0")
        else:
            assert fill.shape == (rows, stride)
            self.tensor = torch.from_numpy(np.ascontiguousarray(fill)).to("cuda:0")
        self.pointer, self.shape = self.tensor.data_ptr(), (rows, stride)
        torch.cuda.synchronize()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.tensor.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def wrong_rows(big, seven):
    """Rows of `big` that are not, bit for bit, row l % 7 of `seven`."""
    rows = np.ascontiguousarray(big).view(np.uint64)
    expect = np.ascontiguousarray(seven).view(np.uint64)[np.arange(big.shape[0]) % cases.K]
    return np.flatnonzero(np.any(rows != expect, axis=1))


def assert_tiled(big, seven, label):
    assert big.shape == (big.shape[0], seven.shape[1]), label
    assert np.isfinite(big).all(), label
    wrong = wrong_rows(big, seven)
    assert wrong.size == 0, f"{label}: rows {wrong[:6]} ... of {wrong.size} are not the rows of " \
                            f"the seven-level call (passes start at {cases.ROW}, {2*cases.ROW})"


def compute(engine, name, count, **kw):
    grid = cases.GRIDS[name]
    t, p, x = cases.levels(count)
    out = engine.compute(engine.handle_of(name), t, p, x, grid.v0, grid.vn, grid.n_per_v,
                         cut_off=grid.cut_off, **kw)
    if isinstance(out, tuple):
        return np.array(out[0]), out[1]
    return np.array(out)        # (the page-locked array is recycled by the next call)


_oracle_rows = {}


def oracle_rows(oracle, name, remove_pedestal=False):
    key = (name, remove_pedestal)
    if key not in _oracle_rows:
        grid = cases.GRIDS[name]
        rows = np.stack([oracle.absorption_port(cases.table(name), t, p, x, grid.v0, grid.vn,
                                                grid.n_per_v, cut_off=grid.cut_off,
                                                remove_pedestal=remove_pedestal)[0]
                         for t, p, x in cases.PATTERN])
        rows.setflags(write=False)
        _oracle_rows[key] = rows
    return _oracle_rows[key]


def meets_the_oracle(oracle, name, seven, label, remove_pedestal=False, scale=None):
    """The seven-level call per level under assert_spectrum; a pedestal spectrum with the plain one
    handed in (tests/test_gpu_pedestal_many_runs.py::_meets_the_oracle)."""
    grid = cases.GRIDS[name]
    case = golden_io.Case("many levels", 0, 0, 0, 0, grid.v0, grid.vn, grid.n_per_v, grid.cut_off,
                          remove_pedestal, None, 0)
    reference = oracle_rows(oracle, name, remove_pedestal)
    plain = oracle_rows(oracle, name)
    for level in range(cases.K):
        factor = 1. if scale is None else scale[level]
        assert_spectrum(seven[level], factor*reference[level], case, f"{label} level {level}",
                        factor*plain[level] if remove_pedestal else None)


def density():
    from pylbl_amd import number_density
    return number_density(cases.PATTERN[:, 0], cases.PATTERN[:, 1], cases.PATTERN[:, 2])


# ---------------------------------------------------------------------------------------------
# Part 1.
@pytest.mark.parametrize("name", ["small", "split", "scan"])
def test_plain_rows_of_every_level_count(engine, oracle, name):
    """Host output.  Every level count; then passes of 20 000 levels through a small
    workspace_bytes: the same bits; and a second call."""
    seven = compute(engine, name, cases.K)
    meets_the_oracle(oracle, name, seven, name)
    for count in cases.COUNTS:
        big = compute(engine, name, count)
        assert_tiled(big, seven, f"{name}, {count} levels")
    assert same_bits(compute(engine, name, cases.COUNTS[-1]), big), "a second call"
    engine.set_option("workspace_bytes", cases.small_workspace(cases.table(name), cases.GRIDS[name],
                                                               False, False))
    try:
        assert_tiled(compute(engine, name, cases.ROW + 12), seven, f"{name}, passes of 20 000")
    finally:
        engine.set_option("workspace_bytes", cases.WORKSPACE)


def test_passes_are_the_caps(engine):
    """With workspace_bytes = 64 GiB a call runs in ceil(levels/65535) passes -- one prologue and
    one accumulate launch each, counted by the engine's own timing (option timing = 1) -- and in
    passes of 20 000 levels under the small budget.  (The results alone would not tell: this
    runtime launches gridDim.y = 131 073 as well, and with the 65535 taken out of levels_per_pass
    every other test of this file passes.)"""
    def launches(count):
        engine.timing(reset=True)
        compute(engine, "small", count)
        counted = engine.timing(reset=True)[1]
        return counted[0], counted[2]       # prepare (prologue), accumulate
    engine.set_option("timing", 1)
    try:
        for count in (cases.K,) + cases.COUNTS:
            passes = -(-count//cases.ROW)
            assert launches(count) == (passes, passes), count
        engine.set_option("workspace_bytes", cases.small_workspace(
            cases.table("small"), cases.SMALL, False, False))
        passes = -(-(cases.ROW + 12)//cases.PASS_LEVELS)
        assert passes == 4 and launches(cases.ROW + 12) == (passes, passes)
    finally:
        engine.set_option("workspace_bytes", cases.WORKSPACE)
        engine.set_option("timing", 0)


def test_scale_density(engine, oracle):
    seven = compute(engine, "small", cases.K, scale_density=True)
    meets_the_oracle(oracle, "small", seven, "n k", scale=density())
    for count in (cases.ROW + 1, 2*cases.ROW + 3):
        assert_tiled(compute(engine, "small", count, scale_density=True), seven, f"n k, {count}")


def test_far_field_series(engine, oracle):
    """LBL_FARFIELD on the grid where shape_of keeps the series on: farfield_series_kernel at
    gridDim.y == 65535 and in the later passes."""
    seven = compute(engine, "far", cases.K, farfield=True)
    meets_the_oracle(oracle, "far", seven, "far")
    assert not same_bits(seven, compute(engine, "far", cases.K)), "the series sums nothing"
    for count in (cases.ROW, cases.ROW + 12):
        assert_tiled(compute(engine, "far", count, farfield=True), seven, f"far, {count} levels")


@pytest.mark.parametrize("name", ["small", "scan"])
def test_pedestal_serial_chain(engine, oracle, name):
    """remove_pedestal with scan_chain = 0 on a poisoned workspace: run_find_kernel (with its
    look-back over three blocks per level for `scan`), run_sums_kernel, run_chain_kernel (level =
    blockIdx.x) and pedestal_apply_kernel at 65535 levels and in the later passes."""
    plain = compute(engine, name, cases.K)
    _options(engine, 0, 0, 1)
    try:
        seven = compute(engine, name, cases.K, remove_pedestal=True)
        meets_the_oracle(oracle, name, seven, f"{name} serial", remove_pedestal=True)
        assert not same_bits(seven, plain)
        counts = cases.COUNTS if name == "small" else (cases.ROW + 12,)
        for count in counts:
            big = compute(engine, name, count, remove_pedestal=True)
            assert_tiled(big, seven, f"{name} serial, {count} levels")
        assert same_bits(compute(engine, name, counts[-1], remove_pedestal=True), big)
        engine.set_option("workspace_bytes", cases.small_workspace(
            cases.table(name), cases.GRIDS[name], False, True))
        assert_tiled(compute(engine, name, cases.ROW + 12, remove_pedestal=True), seven,
                     f"{name} serial, passes of 20 000")
    finally:
        engine.set_option("workspace_bytes", cases.WORKSPACE)
        _options(engine, 1, 0, 0)


@pytest.mark.parametrize("name", ["small", "split"])
def test_pedestal_relaxation(engine, oracle, name):
    """remove_pedestal with the relaxation (the default) on a poisoned workspace: run_links_kernel
    and run_solve_kernel at 65535 levels.  Bit for bit where every pass holds all seven pattern
    levels; a pass of one or three levels may take another number of sweeps (relax_launches
    follows the pass's max_runs): those counts meet the serial chain within 1e-7 of the plain
    spectrum, the bound of tests/test_gpu_pedestal_many_runs.py, and through it the oracle."""
    plain = compute(engine, name, cases.K)
    _options(engine, 0, 0, 1)
    serial = compute(engine, name, cases.K, remove_pedestal=True)
    _options(engine, 1, 0, 1)
    try:
        seven = compute(engine, name, cases.K, remove_pedestal=True)
        meets_the_oracle(oracle, name, seven, f"{name} relaxation", remove_pedestal=True)
        for count in cases.WHOLE_PATTERN_COUNTS:
            big = compute(engine, name, count, remove_pedestal=True)
            assert_tiled(big, seven, f"{name} relaxation, {count} levels")
        assert same_bits(compute(engine, name, count, remove_pedestal=True), big)
        scale = np.maximum(plain, 1e-300)
        for count in (cases.ROW + 1, 2*cases.ROW + 3):
            big = compute(engine, name, count, remove_pedestal=True)
            assert np.isfinite(big).all()
            index = np.arange(count) % cases.K
            apart = float(np.max(np.abs(big - serial[index])/scale[index]))
            print(f"{name} relaxation, {count} levels: {apart:.3g} of the plain spectrum from serial; "
                  f"{wrong_rows(big, seven).size} rows with other bits than the seven-level call")
            assert apart < 1.e-7, (name, count)
    finally:
        _options(engine, 1, 0, 0)


def _raw(engine, name, count, flags, pointer, stride, remove_pedestal=False, evals=None):
    grid = cases.GRIDS[name]
    t, p, x = cases.levels(count)
    status = engine.lib.lbl_compute(
        engine.handle, engine.handle_of(name), count, t.ctypes.data, p.ctypes.data, x.ctypes.data,
        grid.v0, grid.vn, grid.n_per_v, grid.cut_off, int(remove_pedestal), 0, flags,
        c_void_p(pointer), c_int64(stride), evals)
    engine._check(status)


@pytest.mark.parametrize("name,remove_pedestal", [("small", False), ("split", False),
                                                  ("small", True)])
def test_block_in_hbm_with_padded_rows(engine, name, remove_pedestal):
    """LBL_OUT_DEVICE with level_stride > n: `k + base*stride` of the later passes (pass_of) and
    `level*stride` in the kernels.  Padding columns and the rows past the call keep their
    sentinel."""
    from pylbl_amd.engine import OUT_DEVICE
    n = cases.points(cases.GRIDS[name])
    stride = n + 5
    seven = compute(engine, name, cases.K, remove_pedestal=remove_pedestal)
    for count in (cases.ROW + 1, 2*cases.ROW + 3):
        block = Block(count + 2, stride, SENTINEL)
        _raw(engine, name, count, OUT_DEVICE, block.pointer, stride, remove_pedestal)
        got = block.host()
        del block
        assert_tiled(got[:count, :n], seven, f"{name} in HBM, {count} levels")
        assert np.all(got[:count, n:] == SENTINEL) and np.all(got[count:] == SENTINEL)


@pytest.mark.parametrize("remove_pedestal", [False, True])
def test_accumulate(engine, remove_pedestal):
    """LBL_ACCUMULATE: into host rows (the host adds, pass by pass) and into a block in HBM -- with
    the pedestal through lane.raw and pedestal_apply_kernel's own addition.  A row is what was
    there plus the row of the plain call, exactly."""
    from pylbl_amd.engine import ACCUMULATE, OUT_DEVICE
    name, count = "small", cases.ROW + 12
    n = cases.points(cases.GRIDS[name])
    seven = compute(engine, name, cases.K, remove_pedestal=remove_pedestal)
    index = np.arange(count) % cases.K
    before = np.random.default_rng(7).uniform(0., float(seven.max()), (count, n))
    out = before.copy()
    t, p, x = cases.levels(count)
    grid = cases.GRIDS[name]
    engine.compute(engine.handle_of(name), t, p, x, grid.v0, grid.vn, grid.n_per_v,
                   cut_off=grid.cut_off, remove_pedestal=remove_pedestal, accumulate=True, out=out)
    assert same_bits(out, before + seven[index]), "host rows"
    there = np.vstack([before, np.full((1, n), SENTINEL)])
    block = Block(count + 1, n, there)
    _raw(engine, name, count, OUT_DEVICE | ACCUMULATE, block.pointer, n, remove_pedestal)
    got = block.host()
    del block
    assert same_bits(got[:count], before + seven[index]), "block in HBM"
    assert np.all(got[count:] == SENTINEL)


@pytest.mark.parametrize("remove_pedestal", [False, True])
def test_streamed_call_in_pieces(engine, remove_pedestal):
    """lbl_compute_streamed with pieces > 1: every pass delivers its rows (`f.host +
    p.base*f.host_pitch`), the block and the delivered columns are the seven-level rows."""
    from pylbl_amd.engine import DeviceSpectra
    name, count = "pieces", cases.ROW + 12
    n = cases.points(cases.GRIDS[name])
    assert cases.tiling(cases.GRIDS[name], 0).n_tiles > 1
    seven = compute(engine, name, cases.K, remove_pedestal=remove_pedestal)
    out = DeviceSpectra(engine, count, n)
    target = engine.host_array((count, n - 5))
    target[...] = SENTINEL
    try:
        t, p, x = cases.levels(count)
        grid = cases.GRIDS[name]
        engine.compute(engine.handle_of(name), t, p, x, grid.v0, grid.vn, grid.n_per_v,
                       cut_off=grid.cut_off, remove_pedestal=remove_pedestal, out=out,
                       deliver=target, pieces=4)
        engine.synchronize()
        assert_tiled(out.to_host(), seven, "the block")
        assert_tiled(np.array(target), seven[:, :n - 5], "the delivered columns")
    finally:
        out.free()


def test_prep_on_the_host(engine, oracle):
    """LBL_PREP_HOST: prepare_on_host and schedule_kernel in every pass.  (The host's pow and exp
    are not the device's: the project holds both prologues to the oracle, tests/test_gpu_parity.py,
    and claims no equality of bits between them; so does this test, and the big calls are the
    rows of the seven-level call made the same way.)"""
    engine.set_option("prep", 1)
    try:
        seven = compute(engine, "small", cases.K)
        meets_the_oracle(oracle, "small", seven, "host prep")
        for count in (cases.ROW + 1, cases.ROW + 12):
            assert_tiled(compute(engine, "small", count), seven, f"host prep, {count} levels")
    finally:
        engine.set_option("prep", 0)


@pytest.mark.parametrize("prep", [0, 1])
def test_evals(engine, prep):
    """`evals` of a big call is the seven-level call's count per pattern level, multiplied out."""
    engine.set_option("prep", prep)
    try:
        per_level = [compute(engine, "small", 1 + level, want_evals=True)[1]
                     for level in range(cases.K)]
        per_level = np.diff([0] + per_level)
        assert per_level.min() > 0 and len(set(per_level.tolist())) > 1
        for count in (cases.ROW, cases.ROW + 1, 2*cases.ROW + 3):
            _, evals = compute(engine, "small", count, want_evals=True)
            assert evals == int(np.sum(per_level[np.arange(count) % cases.K])), count
    finally:
        engine.set_option("prep", 0)


# ---------------------------------------------------------------------------------------------
# Part 3.
MANY = cases.ROW + 3


def _spectroscopy(count, directory):
    from pylbl_amd import MemoryDatabase, Spectroscopy, arts_crossfit, synthetic
    bands = synthetic.cross_section_bands(seed=5, ranges=((2295., 2303.), (2302., 2312.)),
                                          spacing=0.05)
    arts_crossfit.write_npz(directory / "CFC11.npz", bands)
    co2 = cases.table("small")
    h2o = synthetic.line_table("H2O", 2290., 2318., num_lines=40, seed=77, tips_range=(150, 400))
    database = MemoryDatabase([h2o, co2], cross_sections={"CFC11": str(directory / "CFC11.npz")})
    t, p, x = cases.levels(count)
    index = np.arange(count) % cases.K
    gases = {"H2O": np.asarray([1e-6, 0.02, 0.01, 0.015, 1e-5, 1e-3, 4e-4])[index], "CO2": x,
             "CFC11": np.asarray([2.3e-10, 1e-10, 3e-10, 2e-10, 1e-11, 5e-10, 4e-10])[index]}
    grid = np.arange(cases.SMALL.v0, cases.SMALL.vn, 1./cases.SMALL.n_per_v)
    return Spectroscopy(synthetic.Atmos(p=p, t=t, vmr=gases), grid, database)


@pytest.mark.parametrize("output_format", ["total", "gas", "all"])
def test_compute_absorption_of_65538_levels(tmp_path, output_format):
    """Two gases with lines, the two banded continua of H2O (continua_into takes the group call),
    CO2's own, one cross-section; device routes (16.8 MB a block)."""
    from pylbl_amd.mt_ckd import BandedContinuum
    few, many = _spectroscopy(cases.K, tmp_path), _spectroscopy(MANY, tmp_path)
    continua = many._molecule("H2O").gas_continua
    assert len(continua) == 2 and all(isinstance(c, BandedContinuum) for c in continua)
    assert many._molecule("CFC11").cross_section is not None
    assert MANY*many.grid.size*8 <= many.device_output_limit
    expect = few.compute_absorption(output_format)
    got = many.compute_absorption(output_format)
    names = ["absorption"] if output_format == "total" else \
        [f"{gas}_absorption" for gas in ("H2O", "CO2", "CFC11")]
    for variable in names:
        a, b = np.asarray(got[variable]), np.asarray(expect[variable])
        assert a.shape == (MANY,) + b.shape[1:] and np.isfinite(a).all() and a.any()
        assert_tiled(a.reshape(MANY, -1), b.reshape(cases.K, -1), f"{output_format} {variable}")
    if output_format == "all":
        h2o = np.asarray(got["H2O_absorption"])
        assert h2o[:, 0].any() and h2o[:, 1].any() and not h2o[:, 2].any()
        assert np.asarray(got["CFC11_absorption"])[:, 2].any()


def test_group_of_continua_over_65537_levels(engine):
    """Engine.continuum_compute_many on 65 537 levels against one spectra_levels(...,
    accumulate=True) per continuum: the equality mt_ckd.spectra_levels_many documents, in the
    second run of levels as in the first; written and added to."""
    from pylbl_amd import mt_ckd
    from pylbl_amd.engine import DeviceSpectra
    count = cases.ROW + 2
    members = [mt_ckd.WaterVaporForeignContinuum(engine=engine),
               mt_ckd.WaterVaporSelfContinuum(engine=engine)]
    grid = np.asarray([-15., 0., 2.5, 700., 2200., 4500., 9000.])
    t, p, x = cases.levels(count)
    index = np.arange(count) % cases.K
    vmr = {"H2O": np.asarray([1e-6, 0.02, 0.01, 0.015, 1e-5, 1e-3, 4e-4])[index], "CO2": x,
           "O2": np.full(count, 0.209), "N2": np.full(count, 0.78)}
    together, apart = DeviceSpectra(engine, count, grid.size), DeviceSpectra(engine, count, grid.size)
    try:
        for adding in (False, True):
            if adding:
                for block in (together, apart):
                    members[0].spectra_levels(t, p, vmr, grid, out=block)
            mt_ckd.spectra_levels_many(members, t, p, vmr, grid, together, accumulate=adding)
            for i, member in enumerate(members):
                member.spectra_levels(t, p, vmr, grid, out=apart, accumulate=adding or i > 0)
            a, b = together.to_host(), apart.to_host()
            assert np.isfinite(a).all() and a.any()
            assert same_bits(a, b), f"adding={adding}"
            assert wrong_rows(a, a[:cases.K]).size == 0
    finally:
        together.free()
        apart.free()


# ---------------------------------------------------------------------------------------------
# Part 2.
PAD = 64            # doubles behind the row: they keep their sentinel


class BigRow(object):
    """One row of the largest grid in HBM (8.6 GB), pre-filled, with PAD doubles behind it."""
    def __init__(self):
        import torch
        self.n = cases.points(cases.BIG)
        self.tensor = torch.full((self.n + PAD,), SENTINEL, dtype=torch.float64, device="cuda:0")
        self.pointer = self.tensor.data_ptr()
        torch.cuda.synchronize()

    def refill(self):
        import torch
        self.tensor.fill_(SENTINEL)
        torch.cuda.synchronize()

    def nonzero(self, first, last):
        import torch
        return int(torch.count_nonzero(self.tensor[first:last + 1]).item())

    def slice(self, first, last):
        return self.tensor[first:last + 1].cpu().numpy()

    def padding_kept(self):
        import torch
        return bool(torch.all(self.tensor[self.n:] == SENTINEL).item())


def _big_call(engine, handle, row, flags, remove_pedestal=False):
    grid = cases.BIG
    t, p, x = (np.asarray([v], dtype=np.float64) for v in cases.BIG_LEVEL)
    status = engine.lib.lbl_compute(
        engine.handle, handle, 1, t.ctypes.data, p.ctypes.data, x.ctypes.data, grid.v0, grid.vn,
        grid.n_per_v, grid.cut_off, int(remove_pedestal), 0, flags, c_void_p(row.pointer),
        c_int64(row.n + PAD), None)
    engine._check(status)


def _big_reference(oracle):
    """Per cluster: (first, last) of its merged windows and the float64 sum of oracle.voigt_port
    over every line whose window reaches it, on v[i] = v0 + i*dv.  The windows are the restated
    first / last of the oracle's own centres (the host test holds them to spectra.c:48-62)."""
    table, grid = cases.big_table(), cases.BIG
    t, p, x = cases.BIG_LEVEL
    _, extras = oracle.absorption_port(table, t, p, x, grid.v0, grid.vn, 1, cut_off=grid.cut_off,
                                       want_derived=True)
    derived = extras["derived"]
    first, last, status = cases.windows(derived[:, 0], grid)
    merged, gaps = cases.covered(first, last, status, cases.points(grid))
    clusters = []
    for a, b in merged:
        v = cases.wavenumbers(grid, a, b)
        k = np.zeros(v.size)
        for row in np.flatnonzero((status == 1) & (last >= a) & (first <= b)):
            oracle.voigt_port(v, int(max(first[row], a) - a), int(min(last[row], b) - a),
                              derived[row, 0], derived[row, 1], derived[row, 2], derived[row, 3],
                              k=k)
        clusters.append((a, b, k))
    return clusters, gaps


def _against_the_reference(row, clusters, gaps, label, worst):
    case = golden_io.Case("largest grid", 0, 0, 0, 0, cases.BIG.v0, cases.BIG.vn,
                          cases.BIG.n_per_v, cases.BIG.cut_off, False, None, 0)
    for a, b in gaps:
        assert row.nonzero(a, b) == 0, f"{label}: nonzero outside every window, in [{a}, {b}]"
    assert row.padding_kept(), label
    slices = []
    for c, (a, b, k_ref) in enumerate(clusters):
        k = row.slice(a, b)
        assert np.isfinite(k).all()
        live = k_ref != 0.
        worst[label, c] = float(np.max(np.abs(k[live] - k_ref[live])/k_ref[live]))
        print(f"{label}, cluster {c} [{a}, {b}]: max relative error {worst[label, c]:.3g}")
        slices.append(k)
    for c, (a, b, k_ref) in enumerate(clusters):
        assert_spectrum(slices[c], k_ref, case, f"{label}, cluster {c} at index {a}")
    return slices


def test_largest_grid(oracle):
    """1 073 709 056 points, one level, 40 lines in five clusters on the indices 0, 2^28, 2^29,
    3 2^28 and n - 1: four calls into one 8.6 GB row in HBM -- four points per lane, eight, the
    far-field series (eight, cell-aligned tiles), and the pedestal at four.  Every point outside
    every window is exactly 0.0 (counted on the device); every cluster's slice meets the float64
    sum of oracle.voigt_port at assert_spectrum's plain bar.  The project claims no equality of
    bits between tilings (tests/test_gpu_parity.py::test_golden_every_tile_size holds each to the
    golden vectors): both are held to the oracle and their distance is printed.  With the
    pedestal: 0.0 wherever no window reaches, and in every cell of a cluster away from the
    grid's end k_plain - k_ped is one value on the interior points and one on the integer point,
    within 4 roundings (2^-53 each) of k_plain[i] -- k_ped is one subtraction from k_plain
    (pedestal_apply_kernel), the difference a second one, at the point itself and at the cell's
    point of least k_plain that the value is read from."""
    from pylbl_amd.engine import Engine, FARFIELD, OUT_DEVICE
    started = time.perf_counter()
    engine = Engine(0)
    handle = engine.load(cases.big_table())
    clusters, gaps = _big_reference(oracle)
    print(f"reference: {time.perf_counter() - started:.2f} s")
    row = BigRow()
    worst = {}
    try:
        plain = {}
        for forced in (4, 8):
            engine.set_option("points_per_lane", forced)
            begin = time.perf_counter()
            _big_call(engine, handle, row, OUT_DEVICE)
            print(f"P = {forced}: call {time.perf_counter() - begin:.2f} s")
            plain[forced] = _against_the_reference(row, clusters, gaps, f"P = {forced}", worst)
            row.refill()
        apart = max(float(np.max(np.abs(a - b)/np.maximum(a, 1e-300)))
                    for a, b in zip(plain[4], plain[8]))
        print(f"P = 4 against P = 8: {apart:.3g} relative at most")
        engine.set_option("points_per_lane", 0)
        begin = time.perf_counter()
        _big_call(engine, handle, row, OUT_DEVICE | FARFIELD)
        print(f"far-field series: call {time.perf_counter() - begin:.2f} s")
        far = _against_the_reference(row, clusters, gaps, "far-field series", worst)
        assert any(not same_bits(a, b) for a, b in zip(far, plain[8])), "the series summed nothing"
        row.refill()
        engine.set_option("points_per_lane", 4)
        begin = time.perf_counter()
        _big_call(engine, handle, row, OUT_DEVICE, remove_pedestal=True)
        print(f"pedestal: call {time.perf_counter() - begin:.2f} s")
        for a, b in gaps:
            assert row.nonzero(a, b) == 0, f"pedestal: nonzero outside every window, [{a}, {b}]"
        assert row.padding_kept()
        npv = cases.BIG.n_per_v
        for c, (a, b, _) in enumerate(clusters[:-1]):
            k_ped, k_plain = row.slice(a, b), plain[4][c]
            assert np.isfinite(k_ped).all()
            assert a % npv == 0 and (b - a) % npv == 0      # whole cells and the closing point
            cells = (b - a)//npv
            d = (k_plain - k_ped)[:cells*npv].reshape(cells, npv)
            k = k_plain[:cells*npv].reshape(cells, npv)
            least = np.argmin(k[:, 1:], axis=1) + 1
            value = d[np.arange(cells), least]
            allowed = 2.*2.**-53*(k[:, 1:] + k[np.arange(cells), least][:, None])
            off = np.abs(d[:, 1:] - value[:, None])/allowed
            print(f"pedestal, cluster {c}: interior points within {off.max():.3g} of the bound; "
                  f"pedestals of {value.min():.3g} .. {value.max():.3g}")
            assert off.max() <= 1., c
            # (the integer point also lies in the window that closes on it: no less is taken off)
            assert (value > 0.).any(), c
            assert np.all(d[:, 0] - value >= -2.*2.**-53*(k[:, 0] + k[np.arange(cells), least])), c
    finally:
        import torch
        del row
        torch.cuda.empty_cache()        # the 8.6 GB go back to the device, not to torch's pool
        engine.close()
    print(f"test_largest_grid: {time.perf_counter() - started:.1f} s")


def test_largest_grid_plus_one_cell_is_refused():
    """vn - v0 = 32 768 at 32 768 points per cm-1 is 2^30 points: LBL_BAD_ARGUMENT before anything
    is reserved or written."""
    from pylbl_amd.engine import Engine, EngineError, OUT_DEVICE
    engine = Engine(0)
    handle = engine.load(cases.big_table())
    block = Block(1, 64, SENTINEL)
    grid = cases.REFUSED
    t, p, x = (np.asarray([v], dtype=np.float64) for v in cases.BIG_LEVEL)
    try:
        begin = time.perf_counter()
        status = engine.lib.lbl_compute(
            engine.handle, handle, 1, t.ctypes.data, p.ctypes.data, x.ctypes.data, grid.v0,
            grid.vn, grid.n_per_v, grid.cut_off, 0, 0, OUT_DEVICE, c_void_p(block.pointer),
            c_int64(0), None)
        assert status == 2 and time.perf_counter() - begin < 0.5
        with pytest.raises(EngineError, match=r"status 2: grid has more than 2\^30 points\."):
            engine._check(status)
        assert np.all(block.host() == SENTINEL)
    finally:
        engine.close()
