"""Spectroscopy.compute_path on the GPU against numpy applied to compute_absorption("total") of
the same Spectroscopy (itself pinned to the oracle by the rest of the suite): optical depth bit
for bit in the stated order of additions, transmittance and band means to rounding, runs of
levels, determinism, threads and the C ABI's argument checks."""
import threading

import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic

pytestmark = pytest.mark.gpu

GASES = ("H2O", "CO2", "O3")


def tables(v_lo, v_hi, num_lines):
    return [synthetic.line_table(name, v_lo, v_hi, num_lines=num_lines, seed=40 + i)
            for i, name in enumerate(GASES)]


def atmosphere(shape):
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    return synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                           vmr={k: full.vmr[k].reshape(shape) for k in GASES})


_TABLES = {}


def spectroscopy(shape=(5,), grid=None, **keywords):
    if "small" not in _TABLES:
        _TABLES["small"] = tables(576., 724., 3000)
    grid = np.arange(600., 700., 0.01) if grid is None else grid
    return Spectroscopy(atmosphere(shape), grid, MemoryDatabase(_TABLES["small"]), **keywords)


def lengths_for(shape, seed=0, beta=None):
    """Path lengths [m]; with `beta` scaled so that |tau| stays below ~30 (exp(-tau) finite)."""
    rng = np.random.default_rng(seed)
    lengths = rng.uniform(0.5, 1.5, size=shape)
    if beta is not None:
        scale = np.max(np.sum(np.abs(beta), axis=-2))
        lengths *= 20./scale if scale > 0. else 1.
    return lengths


def numpy_tau(beta, lengths, cumulative):
    """beta [..., L, columns], lengths [..., L]: tau in the order compute_path promises."""
    levels = beta.shape[-2]
    out = np.zeros(beta.shape) if cumulative else None
    tau = np.zeros(beta.shape[:-2] + beta.shape[-1:])
    order = range(levels - 1, -1, -1) if cumulative == "from_last" else range(levels)
    for l in order:
        tau = tau + lengths[..., l, None]*beta[..., l, :]
        if cumulative:
            out[..., l, :] = tau
    return out if cumulative else tau


def numpy_band_means(values, starts):
    means = np.full(values.shape[:-1] + (starts.size - 1,), np.nan)
    for b in range(starts.size - 1):
        if starts[b + 1] > starts[b]:
            means[..., b] = values[..., starts[b]:starts[b + 1]].mean(axis=-1)
    return means


def total_of(spec, remove_pedestal=None):
    return np.asarray(spec.compute_absorption("total", remove_pedestal=remove_pedestal)["absorption"])


def assert_relative(got, expect, bound):
    got, expect = np.asarray(got), np.asarray(expect)
    assert got.shape == expect.shape
    assert np.array_equal(np.isnan(got), np.isnan(expect))
    ok = ~np.isnan(expect)
    error = np.abs(got[ok] - expect[ok])/np.maximum(np.abs(expect[ok]), 1.e-300)
    assert error.size == 0 or error.max() <= bound, error.max()


@pytest.mark.parametrize("remove_pedestal, farfield", [(False, True), (True, True), (True, False),
                                                       (False, False)])
@pytest.mark.parametrize("cumulative", [None, "from_first", "from_last"])
def test_optical_depth_is_the_numpy_loop_bit_for_bit(remove_pedestal, farfield, cumulative):
    spec = spectroscopy((3, 5), farfield=farfield)
    beta = total_of(spec, remove_pedestal)
    lengths = lengths_for((3, 5), beta=beta)
    out = spec.compute_path(lengths, cumulative=cumulative, remove_pedestal=remove_pedestal)
    tau = numpy_tau(beta, lengths, cumulative)
    assert np.array_equal(out["wavenumber"], spec.grid)
    assert out["optical_depth"].shape == tau.shape
    assert np.array_equal(out["optical_depth"], tau)
    assert_relative(out["transmittance"], np.exp(-tau), 1.e-15)


def test_one_level_paths_of_unit_length_return_the_total():
    spec = spectroscopy((5, 1))
    beta = total_of(spec)
    out = spec.compute_path(np.ones((5, 1)), quantities="optical_depth")
    assert set(out) == {"wavenumber", "optical_depth"}
    assert np.array_equal(out["optical_depth"], beta[:, 0, :])


def test_zero_lengths_leave_their_terms_out():
    spec = spectroscopy((5,))
    beta = total_of(spec)
    lengths = lengths_for(5, seed=3, beta=beta)
    lengths[[1, 3]] = 0.
    out = spec.compute_path(lengths, quantities="optical_depth", cumulative="from_first")
    tau = np.zeros(spec.grid.size)
    expect = np.zeros_like(beta)
    for l in range(5):
        if lengths[l] != 0.:
            tau = tau + lengths[l]*beta[l]
        expect[l] = tau
    assert np.array_equal(out["optical_depth"], expect)
    zero = spec.compute_path(np.zeros(5))
    assert np.all(zero["optical_depth"] == 0.)
    assert np.all(zero["transmittance"] == 1.)


@pytest.mark.parametrize("remove_pedestal", [False, True])
@pytest.mark.parametrize("cumulative", [None, "from_first", "from_last"])
def test_band_means(remove_pedestal, cumulative):
    spec = spectroscopy((3, 5))
    grid = spec.grid
    beta = total_of(spec, remove_pedestal)
    lengths = lengths_for((3, 5), seed=5, beta=beta)
    tau = numpy_tau(beta, lengths, cumulative)
    edge_sets = {
        "five points": grid[100:400:5] - 0.001,
        "20 cm-1": np.arange(600., 700.1, 20.),
        "whole grid": [500., 800.],
        "outside and empty": [550., 580., 600.5, 600.5005, 601.3, 690., 720.],
        "single points and straddling": np.concatenate([[599.], grid[[7, 8, 4095, 4096, 4097]]
                                                        - 0.001, [650.02, 681.]]),
    }
    for label, edges in edge_sets.items():
        out = spec.compute_path(lengths, band_edges=edges, cumulative=cumulative,
                                remove_pedestal=remove_pedestal)
        starts = np.searchsorted(grid, edges, side="left")
        assert np.array_equal(out["band_points"], np.diff(starts)), label
        assert np.array_equal(out["band_lower"], np.asarray(edges)[:-1])
        assert_relative(out["optical_depth"], numpy_band_means(tau, starts), 1.e-13)
        assert_relative(out["transmittance"], numpy_band_means(np.exp(-tau), starts), 1.e-13)
        if label == "outside and empty":
            assert out["band_points"][0] == 0 and out["band_points"][2] == 0
            assert np.all(np.isnan(out["transmittance"][..., [0, 2]]))


@pytest.mark.parametrize("cumulative", [None, "from_first", "from_last"])
def test_runs_of_levels_give_the_same_bits(cumulative):
    spec = spectroscopy((3, 5))
    lengths = lengths_for((3, 5), seed=7, beta=total_of(spec, True))
    edges = np.arange(600., 700.1, 0.37)
    whole = spec.compute_path(lengths, cumulative=cumulative)
    whole_bands = spec.compute_path(lengths, cumulative=cumulative, band_edges=edges)
    v0, vn, n_per_v = synthetic.grid_arguments(spec.grid)
    level_bytes = (vn - v0)*n_per_v*8
    for limit in (0, level_bytes, 3*level_bytes):
        spec.device_output_limit = limit
        chunked = spec.compute_path(lengths, cumulative=cumulative)
        chunked_bands = spec.compute_path(lengths, cumulative=cumulative, band_edges=edges)
        for q in ("optical_depth", "transmittance"):
            assert np.array_equal(chunked[q], whole[q]), (limit, q)
            assert np.array_equal(chunked_bands[q], whole_bands[q], equal_nan=True), (limit, q)


def test_repeated_calls_and_threads_give_the_same_bits():
    spec = spectroscopy((3, 5))
    lengths = lengths_for((3, 5), seed=9, beta=total_of(spec, True))
    edges = np.arange(600., 700.1, 1.)
    calls = [dict(), dict(band_edges=edges), dict(cumulative="from_last", band_edges=edges),
             dict(cumulative="from_first")]
    first = [spec.compute_path(lengths, **c) for c in calls]
    for _ in range(2):
        for c, expect in zip(calls, first):
            again = spec.compute_path(lengths, **c)
            for q in ("optical_depth", "transmittance"):
                assert np.array_equal(again[q], expect[q], equal_nan=True)
    got = {}

    def worker(index):
        got[index] = [spec.compute_path(lengths, **c) for c in calls]
    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for index in range(2):
        for result, expect in zip(got[index], first):
            for q in ("optical_depth", "transmittance"):
                assert np.array_equal(result[q], expect[q], equal_nan=True)


def test_c_abi_rejects_bad_arguments_and_stays_usable():
    from pylbl_amd import engine as engine_module
    engine = engine_module.default_engine(0)
    lib = engine.lib
    paths, per_path, n, columns = 2, 3, 64, 60
    beta = engine.blocks.take(paths*per_path, n)
    carry = engine.blocks.take(paths, n)
    tau = engine.blocks.take(paths, n)
    lengths = np.ones(paths*per_path)
    starts = np.array([0, 10, 60], dtype=np.int64)
    TAU, CONT = engine_module.PATH_OPTICAL_DEPTH, engine_module.PATH_CONTINUE

    def call(beta_p=beta.pointer, stride=n, cols=columns, n_paths=paths, levels=per_path,
             begin=0, count=paths*per_path, length=lengths, n_bands=0, band=None,
             carry_p=carry.pointer, tau_p=tau.pointer, flags=TAU):
        return lib.lbl_path_compute(
            engine.handle, beta_p, stride, cols, n_paths, levels, begin, count,
            length.ctypes.data if length is not None else None, n_bands,
            band.ctypes.data if band is not None else None, carry_p, tau_p, None, flags)
    try:
        engine.fill_zero(beta)
        bad = [
            dict(beta_p=None), dict(carry_p=None), dict(tau_p=None), dict(length=None),
            dict(cols=n + 1), dict(cols=0), dict(n_paths=0), dict(levels=0),
            dict(begin=-1), dict(count=0), dict(begin=1, count=paths*per_path),
            dict(begin=1, count=2),                     # inside a path without LBL_PATH_CONTINUE
            dict(begin=3, count=3, flags=TAU | CONT),   # starts a path with it
            dict(flags=0),
            dict(flags=TAU | engine_module.PATH_FROM_LAST),
            dict(length=np.array([1., 1., -1., 1., 1., 1.])),
            dict(length=np.array([1., 1., np.nan, 1., 1., 1.])),
            dict(length=np.array([1., np.inf, 1., 1., 1., 1.])),
            dict(n_bands=2, band=None), dict(n_bands=-1),
            dict(n_bands=2, band=np.array([0, 30, 20], dtype=np.int64)),
            dict(n_bands=2, band=np.array([-1, 10, 20], dtype=np.int64)),
            dict(n_bands=2, band=np.array([0, 10, 61], dtype=np.int64)),
        ]
        for arguments in bad:
            assert call(**arguments) == 2, arguments        # LBL_BAD_ARGUMENT
            assert lib.lbl_last_error(engine.handle).decode().startswith("lbl_path_compute")
        assert call(begin=1, count=2, flags=TAU | CONT) == 0
        assert call(n_bands=2, band=starts) == 0
    finally:
        engine.synchronize()
        for block in (beta, carry, tau):
            engine.blocks.give(block)
    spec = spectroscopy((5,))
    out = spec.compute_path(np.ones(5), quantities="optical_depth")
    assert np.array_equal(out["optical_depth"], numpy_tau(total_of(spec), np.ones(5), None))


def test_large_grid():
    """16 levels on 1-3000 cm-1 at 0.01: ~1200 sweep workgroups per path, bands that straddle
    the 4096-column segments."""
    big = [synthetic.line_table(name, 1., 3000., num_lines=20000, seed=60 + i)
           for i, name in enumerate(GASES)]
    spec = Spectroscopy(atmosphere((16,)), np.arange(1., 3000., 0.01), MemoryDatabase(big))
    beta = total_of(spec)
    lengths = lengths_for(16, seed=11, beta=beta)
    tau = numpy_tau(beta, lengths, None)
    out = spec.compute_path(lengths)
    assert np.array_equal(out["optical_depth"], tau)
    assert_relative(out["transmittance"], np.exp(-tau), 1.e-15)
    edges = np.concatenate([[0.5], np.arange(1.003, 3000., 7.77), [3100.]])
    bands = spec.compute_path(lengths, band_edges=edges, cumulative="from_last")
    starts = np.searchsorted(spec.grid, edges, side="left")
    cum = numpy_tau(beta, lengths, "from_last")
    assert_relative(bands["optical_depth"], numpy_band_means(cum, starts), 1.e-13)
    assert_relative(bands["transmittance"], numpy_band_means(np.exp(-cum), starts), 1.e-13)
