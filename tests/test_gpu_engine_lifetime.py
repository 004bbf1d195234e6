"""What the engine's owner types (csrc/hip_owners.h) decide and no other test looks at: an engine
closed while calls are queued, a handle freed right behind a queued call that uses it, the
page-locked staging blocks refilled (and grown) by a call that follows one still in flight, and
the one failure of lbl_engine_create that needs no fault.  Ordering and lifetime, not arithmetic:
every result is compared bit for bit with the same call made synchronously, on shapes of a few
hundred lines and 128 grid points."""
import numpy as np
import pytest

from pylbl_amd import synthetic
from pylbl_amd.engine import Engine, EngineError
from pylbl_amd.instrument import Instrument

pytestmark = pytest.mark.gpu

V0, VN, NPV, CUT_OFF = 600, 602, 64, 3
N = (VN - V0)*NPV
GRID = V0 + np.arange(N)/NPV
# (The reference's range rule stops at the first row outside v0 - cut_off - 1 ... vn + cut_off + 1:
# the table lies inside.)
TABLE = synthetic.line_table("H2O", V0 - CUT_OFF - 1., VN + CUT_OFF + 1., num_lines=300, seed=5)
_rng = np.random.default_rng(17)
# (kind, lower bound, resolution, columns): kinds 0 and 5 read two columns and one.
CONTINUUM = [(0, 598., 1., [_rng.uniform(1e-25, 2e-25, 8), _rng.uniform(1e-25, 2e-25, 8)]),
             (5, 599., 0.5, [_rng.uniform(1e-25, 2e-25, 12)])]
XSEC = synthetic.cross_section_bands(seed=2, ranges=((598., 604.),), spacing=0.5)
INSTRUMENT = Instrument.gaussian(np.array([600.5, 601., 601.5]), 0.2, half_width=0.4)
BANDS = [0, 64, 128]


def levels(count, shift=0.):
    """(temperature, pressure, one gas's mixing ratio, the continuum's five) of `count` levels."""
    i = np.arange(count)
    t = 220. + 9.*i + shift
    p = 9.e4 - 7.e3*i - 100.*shift
    x = 0.004 + 0.001*i
    five = np.tile([0.01, 0.21, 0.78, 0.01, 1.0], (count, 1))
    five[:, 0] = five[:, 3] = x
    return t, p, x, five


class Rows(object):
    """A float64 torch tensor [rows, row length] on the GPU as a call's block: memory that stays
    valid whatever becomes of the engine."""
    def __init__(self, rows, n):
        import torch
        self.tensor = torch.zeros((rows, n), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        self.pointer, self.shape = self.tensor.data_ptr(), (rows, n)

    def host(self):
        return self.tensor.cpu().numpy().copy()


def pinned(rows, n):
    import torch
    return torch.zeros((rows, n), dtype=torch.float64).pin_memory()


class World(object):
    """One engine with everything the calls below need loaded."""
    def __init__(self, engine):
        self.engine = engine
        self.molecule = engine.load(TABLE)
        self.grid = engine.load_grid(GRID)
        self.continuum = engine.load_continuum(CONTINUUM)
        self.second = engine.load_continuum(CONTINUUM[:1])
        self.xsec = engine.load_xsec(XSEC)
        self.instrument = INSTRUMENT._create(engine, self.grid)

    # Each call: fresh blocks in, {name: block} out.  a: asynchronous.
    def lines(self, a, lv, keep):
        t, p, x, _ = lv
        out = Rows(t.size, N)
        self.engine.compute(self.molecule, t, p, x, V0, VN, NPV, cut_off=CUT_OFF,
                            remove_pedestal=True, out=out, asynchronous=a)
        return {"lines": out}

    def streamed(self, a, lv, keep):
        t, p, x, _ = lv
        out, home = Rows(t.size, N), pinned(t.size, N)
        keep.append(home)
        self.engine.compute(self.molecule, t, p, x, V0, VN, NPV, cut_off=CUT_OFF, out=out,
                            deliver=home.numpy(), pieces=2, asynchronous=a)
        return {"streamed": out, "delivered": home}

    def continuum_one(self, a, lv, keep):
        t, p, _, five = lv
        out = Rows(t.size, N)
        self.engine.continuum_compute(self.continuum, self.grid, N, t, p, five, out=out,
                                      asynchronous=a)
        return {"continuum": out}

    def continuum_many(self, a, lv, keep):
        t, p, _, five = lv
        out = Rows(t.size, N)
        self.engine.continuum_compute_many([self.continuum, self.second], self.grid, N, t, p,
                                           np.stack([five, five]), out=out, asynchronous=a)
        return {"many": out}

    def xsec_one(self, a, lv, keep):
        t, p, x, _ = lv
        out = Rows(t.size, N)
        self.engine.xsec_compute(self.xsec, self.grid, N, t, p, vmr=x, out=out, asynchronous=a)
        return {"xsec": out}

    def path(self, a, beta, lengths, keep, bands=BANDS):
        carry, tau = Rows(1, N), Rows(1, len(bands) - 1)
        keep.append(carry)
        self.engine.path_compute(beta, N, 1, beta.shape[0], 0, lengths, carry, optical_depth=tau,
                                 band_start=bands, asynchronous=a)
        return {"path": tau}

    def channels(self, a, values, keep):
        out = Rows(values.shape[0], 3)
        self.engine.instrument_apply(values, values.shape[0], self.instrument, out,
                                     asynchronous=a)
        return {"channels": out}

    def everything(self, a, keep):
        """Every family of call once, on two levels; the path and the instrument read the lines'
        block."""
        lv = levels(2)
        blocks = {}
        for call in (self.lines, self.streamed, self.continuum_one, self.continuum_many,
                     self.xsec_one):
            blocks.update(call(a, lv, keep))
        blocks.update(self.path(a, blocks["lines"], [1.e24, 2.e24], keep))
        blocks.update(self.channels(a, blocks["lines"], keep))
        keep.append(blocks)
        return blocks


def fetch(engine, blocks):
    engine.synchronize()
    return {name: b.host() if isinstance(b, Rows) else b.numpy().copy()
            for name, b in blocks.items()}


def assert_same(got, expect):
    assert got.keys() == expect.keys()
    for name in expect:
        assert np.all(np.isfinite(expect[name])), name
        assert got[name].tobytes() == expect[name].tobytes(), name


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its GPU state up in 2 s in a process without an engine, in 12 s in one that
    has made an engine already."""
    import torch
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def world():
    engine = Engine(0)
    yield World(engine)
    engine.close()


def test_close_with_work_queued():
    keep = []       # the calls' memory outlives every engine that may still write it
    first = None
    for round in range(8):
        engine = Engine(0)
        w = World(engine)
        if first is None:
            first = fetch(engine, w.everything(True, keep))
        w.everything(True, keep)
        engine.close()      # nothing waited for: the engine drains its own streams
    engine = Engine(0)
    try:
        assert_same(fetch(engine, World(engine).everything(False, keep)), first)
    finally:
        engine.close()
    assert np.any(first["lines"] != 0.) and np.any(first["path"] != 0.)
    assert np.array_equal(first["delivered"], first["streamed"])


FREES = {
    # what is freed: (attribute of World, free, load again, the message of a second free)
    "molecule": ("molecule", "free", lambda e: e.load(TABLE), "unknown molecule handle."),
    "continuum": ("continuum", "free_continuum", lambda e: e.load_continuum(CONTINUUM),
                  "unknown continuum handle."),
    "grid": ("grid", "free_grid", lambda e: e.load_grid(GRID), "unknown grid handle."),
    "xsec": ("xsec", "free_xsec", lambda e: e.load_xsec(XSEC), "unknown cross-section handle."),
    "instrument": ("instrument", "instrument_free", None,
                   "lbl_instrument_free: unknown instrument handle."),
}


@pytest.mark.parametrize("what, call", [("molecule", "lines"), ("continuum", "continuum_one"),
                                        ("continuum", "continuum_many"), ("grid", "continuum_one"),
                                        ("xsec", "xsec_one"), ("instrument", "channels")])
def test_free_right_after_queueing(world, what, call):
    engine, keep = world.engine, []
    attribute, free, load, message = FREES[what]
    if load is None:
        load = lambda e: INSTRUMENT._create(e, world.grid)
    values = world.lines(False, levels(2), keep)["lines"]
    argument = values if call == "channels" else levels(2)
    expect = fetch(engine, getattr(world, call)(False, argument, keep))
    handle = getattr(world, attribute)
    blocks = getattr(world, call)(True, argument, keep)
    getattr(engine, free)(handle)       # at once: the free itself waits for the queued call
    assert_same(fetch(engine, blocks), expect)
    with pytest.raises(EngineError) as second:
        getattr(engine, free)(handle)
    assert str(second.value).endswith(message)
    # The slot is handed out again, and what is loaded into it works.
    setattr(world, attribute, load(engine))
    assert getattr(world, attribute) == handle
    if what == "grid":      # (the instrument was bound to the grid that went)
        engine.instrument_free(world.instrument)
        world.instrument = INSTRUMENT._create(engine, world.grid)
    assert_same(fetch(engine, getattr(world, call)(False, argument, keep)), expect)


@pytest.mark.parametrize("call", ["lines", "continuum_one", "continuum_many", "xsec_one"])
@pytest.mark.parametrize("counts", [(2, 2), (5, 5), (2, 6)])
def test_pinned_block_reuse(world, call, counts):
    """Two calls back to back with different levels: the second refills the block the first
    uploads from -- a larger one for (2, 6).  (Up to four levels of a lines call travel as kernel
    arguments; five and six go through the block.)"""
    keep = []
    pair = [levels(counts[0]), levels(counts[1], shift=3.5)]
    expect = [fetch(world.engine, getattr(world, call)(False, lv, keep)) for lv in pair]
    queued = [getattr(world, call)(True, lv, keep) for lv in pair]
    got = [fetch(world.engine, blocks) for blocks in queued]
    for g, e in zip(got, expect):
        assert_same(g, e)
    assert expect[0][next(iter(expect[0]))].tobytes() != expect[1][next(iter(expect[1]))].tobytes()


@pytest.mark.parametrize("bands", [(BANDS, BANDS), (BANDS, [0, 20, 64, 100, 128])])
def test_path_tables_reuse(world, bands):
    """The same for lbl_path_compute's staged tables: other path lengths, then more bands."""
    keep = []
    beta = world.lines(False, levels(2), keep)["lines"]
    pair = [([1.e24, 2.e24], bands[0]), ([3.e24, 0.5e24], bands[1])]
    expect = [fetch(world.engine, world.path(False, beta, s, keep, bands=b)) for s, b in pair]
    queued = [world.path(True, beta, s, keep, bands=b) for s, b in pair]
    for blocks, e in zip(queued, expect):
        assert_same(fetch(world.engine, blocks), e)
    assert np.all(expect[0]["path"] != 0.)
    assert not np.array_equal(expect[0]["path"][0, :2], expect[1]["path"][0, :2])


def test_creation_failure_message():
    import torch
    with pytest.raises(EngineError, match="device index out of range"):
        Engine(device=torch.cuda.device_count())
    engine = Engine(0)
    try:
        w = World(engine)
        assert np.any(fetch(engine, w.lines(False, levels(2), []))["lines"] != 0.)
    finally:
        engine.close()
