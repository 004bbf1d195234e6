"""Spectroscopy.compute_path within its limits: runs of levels hold one run's block in HBM, not
the whole atmosphere, and atmospheres with more paths (or band-mean rows) than a launch grid's y
dimension takes are done in several runs with the same results.  A run holds at most 65 535 levels
(paths._cut_runs), so each of them is one launch of the sweep and one chunk of band means: the
later launches of a run are reached by tests/test_gpu_many_paths.py, which feeds the entries."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic

pytestmark = pytest.mark.gpu

GASES = ("H2O", "CO2", "O3")


def atmosphere(shape):
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    return synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                           vmr={k: full.vmr[k].reshape(shape) for k in GASES})


def spectroscopy(shape, grid, atmos=None):
    tables = [synthetic.line_table(name, 576., 724., num_lines=3000, seed=40 + i)
              for i, name in enumerate(GASES)]
    atmos = atmosphere(shape) if atmos is None else atmos
    return Spectroscopy(atmos, grid, MemoryDatabase(tables))


def lengths_for(beta, seed):
    """Path lengths [m] that keep |tau| below ~20."""
    lengths = np.random.default_rng(seed).uniform(0.5, 1.5, size=beta.shape[:-1])
    return lengths*20./np.max(np.sum(np.abs(beta), axis=-2))


class Ledger(object):
    """Counts the HBM bytes taken from an engine's block pool and not yet given back."""
    def __init__(self, pool, monkeypatch):
        self.held = self.peak = 0
        take, give = pool.take, pool.give

        def counted_take(levels, n):
            block = take(levels, n)
            self.held += block.shape[0]*block.shape[1]*8
            self.peak = max(self.peak, self.held)
            return block

        def counted_give(block):
            self.held -= block.shape[0]*block.shape[1]*8
            give(block)
        monkeypatch.setattr(pool, "take", counted_take)
        monkeypatch.setattr(pool, "give", counted_give)


@pytest.mark.parametrize("cumulative", [None, "from_first", "from_last"])
@pytest.mark.parametrize("run_levels", [1, 4])
def test_runs_hold_one_run_of_levels(monkeypatch, cumulative, run_levels):
    shape = (3, 5)
    spec = spectroscopy(shape, np.arange(600., 700., 0.01))
    beta = np.asarray(spec.compute_absorption("total")["absorption"])
    lengths = lengths_for(beta, seed=1)
    whole = spec.compute_path(lengths, cumulative=cumulative)
    v0, vn, n_per_v = synthetic.grid_arguments(spec.grid)
    row = (vn - v0)*n_per_v*8
    spec.device_output_limit = run_levels*row
    ledger = Ledger(spec._molecule("H2O").gas.engine.blocks, monkeypatch)
    chunked = spec.compute_path(lengths, cumulative=cumulative)
    paths = shape[0]
    # beta of one run, the carry rows, and per quantity either one run (cumulative) or one row
    # per path -- never the 15 levels of the atmosphere.
    bound = (run_levels + paths + 2*(run_levels if cumulative else paths))*row
    assert ledger.held == 0
    assert 0 < ledger.peak <= bound, (ledger.peak, bound)
    for q in ("optical_depth", "transmittance"):
        assert np.array_equal(chunked[q], whole[q])


@pytest.mark.parametrize("cumulative", [None, "from_first"])
def test_more_paths_than_the_grid_y_limit(cumulative):
    """70 000 paths of two levels: the 140 000 levels take several runs, and the sweep and
    (cumulative: 140 000 rows of) band means one launch in each of them -- a run holds at most
    65 535 levels, so at most 32 768 paths and 65 535 rows of means.  The reference absorption
    comes from four Spectroscopy objects of 17 500 paths each (one call takes at most 65 535
    levels)."""
    shape = (70000, 2)
    grid = np.arange(600., 600.64, 0.01)
    atmos = atmosphere(shape)
    spec = spectroscopy(shape, grid, atmos)
    halves = []
    for part in (slice(p, p + 17500) for p in range(0, 70000, 17500)):
        sub = synthetic.Atmos(p=atmos.p[part], t=atmos.t[part],
                              vmr={k: v[part] for k, v in atmos.vmr.items()})
        halves.append(np.asarray(spectroscopy(None, grid, sub).compute_absorption("total")
                                 ["absorption"]))
    beta = np.concatenate(halves)
    lengths = lengths_for(beta, seed=2)
    out = spec.compute_path(lengths, cumulative=cumulative)
    first = lengths[:, 0, None]*beta[:, 0, :]
    tau = first + lengths[:, 1, None]*beta[:, 1, :]
    expect = np.stack([first, tau], axis=1) if cumulative else tau
    assert np.array_equal(out["optical_depth"], expect)
    edges = [600., 600.2, 600.45, 601.]
    bands = spec.compute_path(lengths, cumulative=cumulative, band_edges=edges)
    starts = np.searchsorted(grid, edges)
    for b in range(3):
        values = expect[..., starts[b]:starts[b + 1]]
        got = bands["optical_depth"][..., b]
        # (tau changes sign inside some bands here -- the pedestal makes beta negative -- so the
        # rounding of a sum is bounded by the mean of |tau|, not by the mean itself)
        scale = np.maximum(np.abs(values).mean(axis=-1), 1.e-300)
        assert np.max(np.abs(got - values.mean(axis=-1))/scale) <= 1.e-13
