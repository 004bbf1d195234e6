"""The host side of the weighted k-distributions without a GPU: the numpy mirror of the contract
(tests/kdistribution_weighted_cases.py) on the value kinds where ties decide, every refusal of the
request (raised before anything touches the GPU), include/lbl_amd_kdist.h against
abi.KDIST_PROTOTYPES, what a weighted and an unweighted call queue on a stand-in engine -- the
unweighted logs are those recorded before the weighting existed,
tests/golden/kdistribution_unweighted_queue.json -- and the fractions and weighted means that
paths._create_kdistribution_dataset forms of the device's sums."""
from collections import namedtuple
import ctypes
import inspect
import json
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, paths
from pylbl_amd import engine as engine_module
from tests import abi_header, kdistribution_cases as cases, kdistribution_weighted_cases as wc
from tests import surface_cases as surface

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd_kdist.h").read_text()
F64, LD = np.float64, np.longdouble
Atmosphere = namedtuple("Atmosphere", ["p", "t", "vmr"])
SHAPE = (2, 3)
GRID = np.arange(1000., 1010., 0.01)


class NoDatabase(object):
    def molecules(self):
        return []


def spectroscopy():
    t = np.linspace(200., 300., 6).reshape(SHAPE)
    atmosphere = Atmosphere(p=np.full(SHAPE, 5.e4), t=t, vmr={"H2O": np.full(SHAPE, 1.e-3)})
    return Spectroscopy(atmosphere, GRID, NoDatabase())


def request(spec, quantities=("absorption_g_mean",), weighting=None, weighting_temperature=None,
            band_edges=(1000., 1005., 1010.), g_edges=16):
    return paths._kdistribution_request(spec, band_edges, g_edges, None, quantities, "reference",
                                        weighting, weighting_temperature)


# ---------------------------------------------------------------------------------------------
# The mirror.
@pytest.mark.parametrize("kind", wc.VALUE_KINDS)
def test_mirror_is_the_stable_argsort_of_the_keys(kind):
    """pi sorts (key, offset) lexicographically: the keys ascend, offsets ascend within equal
    keys, the sorted values are the plain oracle's bits, and pi is a permutation."""
    rng = np.random.default_rng(40 + wc.VALUE_KINDS.index(kind))
    for n in (1, 7, 9, 130, 4097, 6145):
        values = wc.values_of(kind, n, rng)
        order = wc.stable_order(values)
        assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(n))
        keys = cases.keys(values)[order]
        assert np.all(keys[1:] >= keys[:-1])
        assert np.all(np.diff(order.astype(np.int64))[keys[1:] == keys[:-1]] > 0)
        assert cases.same_bits(values[order], cases.key_sort(values))
        pairs = sorted(zip(cases.keys(values).tolist(), range(n)))
        assert [j for _, j in pairs] == order.tolist()
    if kind != "random":
        values = wc.values_of(kind, 4097, rng)
        assert np.unique(cases.keys(values)).size < values.size        # ties: the kind's point


def test_the_pad_key_occurs_among_the_values():
    """The NaN 0x7FFF...F has the greatest key, the key a short chunk is padded with: only the
    pad's offset 2^32 - 1 keeps the padding behind it."""
    assert cases.keys(np.array([wc.MAX_KEY_NAN]))[0] == np.uint64(0xFFFFFFFFFFFFFFFF)
    rng = np.random.default_rng(3)
    for n in (1, 7, 9, 130):
        assert np.any(cases.keys(wc.values_of("nans", n, rng)) == np.uint64(0xFFFFFFFFFFFFFFFF))
    kernels = (ROOT / "pylbl_amd" / "csrc" / "band_sort_pairs.h").read_text()
    assert "kSortPadOffset = 0xFFFFFFFFu" in kernels
    assert "std::numeric_limits<int32_t>::max()" in \
        (ROOT / "pylbl_amd" / "csrc" / "band_sort_pairs_entry.inc").read_text()


def test_mirror_rows_weights_and_sums():
    rng = np.random.default_rng(5)
    starts = np.array([2, 3, 12, 12, 40], dtype=np.int64)
    values = np.stack([wc.values_of("two values", 45, rng), wc.values_of("random", 45, rng)])
    weights = rng.random(45)
    order, ordered = wc.sorted_rows(values, starts)
    assert cases.same_bits(ordered, cases.sort_bands(values, starts))
    assert np.all(order[:, :2] == wc.INDEX_SENTINEL) and np.all(order[:, 40:] == wc.INDEX_SENTINEL)
    w, wk = wc.gathered(order, ordered, starts, weights)
    for r in range(2):
        for b in range(4):
            a, e = starts[b], starts[b + 1]
            assert np.array_equal(w[r, a:e], weights[a:e][order[r, a:e]])
            assert np.array_equal(wk[r, a:e], w[r, a:e]*ordered[r, a:e])
    intervals = wc.flat_intervals(starts, [0., 0.5, 1.])
    assert intervals.tolist() == [2, 3, 3, 3, 8, 12, 12, 12, 12, 12, 26, 40]
    total, size = wc.interval_sums(w, intervals)
    assert total.dtype == LD and total.shape == (2, 11)
    band = wc.per_band(total, 4, 2)
    assert band.shape == (2, 4, 2) and np.all(band[:, 2] == 0)
    assert abs(band[0, 3].sum() - np.sum(weights[12:40].astype(LD))) < 1e-15
    # Planck rows: the stated order in float64 next to the long-double reference; 0 for nu <= 0.
    grid = np.array([-1., 0., 500., 1000.])
    stated = wc.planck_weights(F64, grid, wc.PLANCK_TEMPERATURES)
    exact = wc.planck_weights(LD, grid, wc.PLANCK_TEMPERATURES)
    assert stated.shape == (3, 4) and np.all(stated[:, :2] == 0.) and np.all(stated[:, 2:] > 0.)
    assert np.all(np.abs(stated[:, 2:] - exact[:, 2:]) <= 1e-15*exact[:, 2:])
    assert np.all(np.diff(stated[:, 3]) > 0.)


# ---------------------------------------------------------------------------------------------
# The request.
WEIGHTED = paths.KDISTRIBUTION_WEIGHTED_QUANTITIES
BAD = [
    (dict(weighting="solar"), "weighting must be one of"),
    (dict(weighting=""), "weighting must be one of"),
    (dict(weighting=np.ones(GRID.size - 1)), "one weight per grid point"),
    (dict(weighting=np.ones((2, GRID.size))), "one weight per grid point"),
    (dict(weighting=1.), "one weight per grid point"),
    (dict(weighting=-np.ones(GRID.size)), "finite and >= 0"),
    (dict(weighting=np.full(GRID.size, np.nan)), "finite and >= 0"),
    (dict(weighting=np.full(GRID.size, np.inf)), "finite and >= 0"),
    (dict(weighting_temperature=250.), 'needs weighting="planck"'),
    (dict(weighting=np.ones(GRID.size), weighting_temperature=250.), 'needs weighting="planck"'),
    (dict(weighting="planck", weighting_temperature=0.), "finite and > 0"),
    (dict(weighting="planck", weighting_temperature=-1.), "finite and > 0"),
    (dict(weighting="planck", weighting_temperature=np.nan), "finite and > 0"),
    (dict(weighting="planck", weighting_temperature=np.full(3, 250.)), "shape"),
    (dict(weighting="planck", weighting_temperature=np.full((3, 2), 250.)), "shape"),
    (dict(quantities="weight_g_fraction"), "need a weighting"),
    (dict(quantities="absorption_g_weighted_mean"), "need a weighting"),
    (dict(quantities=("absorption_g_mean", "sorted_column")), "need a weighting"),
    (dict(weighting="planck", quantities="transmittance"), "quantities must be"),
    (dict(weighting="planck", quantities=()), "quantities must be"),
]


@pytest.mark.parametrize("keywords, match", BAD)
def test_bad_arguments_are_refused_before_the_gpu(monkeypatch, keywords, match):
    def touched(*arguments, **more):
        raise AssertionError("the GPU side was reached")
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", touched)
    monkeypatch.setattr(engine_module, "default_engine", lambda device=0: surface.Untouchable())
    spec = spectroscopy()
    with pytest.raises(ValueError, match=match):
        spec.compute_kdistribution([1000., 1005., 1010.], **keywords)
    with pytest.raises(ValueError, match=match):
        request(spec, **keywords)


def test_requests_hold_what_the_sweep_needs():
    spec = spectroscopy()
    plain = request(spec)
    assert plain.weighting is None and plain.weights is None and plain.weight_temperature is None
    own = request(spec, WEIGHTED, "planck")
    assert own.weighting == "planck" and own.weights is None and own.quantities == WEIGHTED
    assert np.array_equal(own.weight_temperature, spec.atmosphere.temperature.ravel())
    assert np.array_equal(request(spec, WEIGHTED, "planck", 255.).weight_temperature, [255.]*6)
    given = np.linspace(210., 260., 6).reshape(SHAPE)
    assert np.array_equal(request(spec, WEIGHTED, "planck", given).weight_temperature,
                          given.ravel())
    weights = np.linspace(0., 2., GRID.size)
    array = request(spec, ("sorted_column", "absorption_g_mean"), weights)
    assert array.weighting == "array" and array.weight_temperature is None
    assert np.array_equal(array.weights, weights) and array.weights.flags.c_contiguous
    assert array.quantities == ("absorption_g_mean", "sorted_column")
    # What is not a weighting stays as it was.
    for name in ("starts", "g_edges", "g_points", "interval_starts", "point_index"):
        assert np.array_equal(getattr(own, name), getattr(plain, name)), name
    signature = list(inspect.signature(Spectroscopy.compute_kdistribution).parameters)
    assert signature == ["self", "band_edges", "g_edges", "g_points", "quantities",
                         "remove_pedestal", "range_policy", "weighting", "weighting_temperature"]
    assert paths.KDISTRIBUTION_QUANTITIES == ("absorption_g_mean", "absorption_g_quantile",
                                              "sorted_absorption")


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_kdist.h against abi.KDIST_PROTOTYPES, whole, as
# tests/test_thermal_host.py compares lbl_amd_thermal.h with abi.THERMAL_PROTOTYPES.
def declarations():
    """{function: [parameter, ...]} of the header, in its order, by abi_header's own pattern."""
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    found = {}
    for result, name, inside in re.findall(
            r"^(int|const char \*|void \*)\s*(lbl_\w+)\s*\(([^)]*)\)\s*;", code, re.M):
        assert result == "int" and name not in found, name
        found[name] = [re.sub(r"\s+", " ", p).strip() for p in inside.split(",")]
    assert set(re.findall(r"\b(lbl_\w+)\s*\(", code)) == set(found)
    return found


def test_header_declares_the_entry_and_ctypes_match():
    from pylbl_amd import abi
    declared = declarations()
    assert list(declared) == list(abi.KDIST_PROTOTYPES) == ["lbl_band_distribution_weighted"]
    entry = declared["lbl_band_distribution_weighted"]
    plain = abi_header.parameters_of("lbl_band_distribution")
    # What lbl_band_distribution takes, in its order, with the additions between.
    assert entry[:8] == plain[:8]
    assert entry[8:16] == ["int32_t grid", "const double *row_temperature",
                           "const double *weight_row", "int32_t *index_rows",
                           "int32_t *index_scratch", "int64_t index_stride",
                           "double *weight_rows", "double *weighted_rows"]
    assert entry[16:18] == plain[8:10]
    assert entry[18:20] == ["double *weight_sums", "double *weighted_sums"]
    assert entry[20:] == plain[10:]
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    for name, parameters in declared.items():
        argtypes = abi.KDIST_PROTOTYPES[name]
        assert len(argtypes) == len(parameters), name
        for argtype, parameter in zip(argtypes, parameters):
            abi_header.check_parameter(argtype, parameter, addresses=True)
        function = getattr(lib, name)
        assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
        assert name not in abi.PROTOTYPES and name not in abi.TWO_STREAM_PROTOTYPES
        assert name not in abi.THERMAL_PROTOTYPES and name not in abi.RESULT_TYPES
    # lbl_amd.h is as it was: the new header includes it and declares nothing of its own twice.
    assert '#include "lbl_amd.h"' in HEADER
    assert not set(declared) & set(abi_header.DECLARATIONS)
    assert callable(engine_module.Engine.band_distribution_weighted)


# ---------------------------------------------------------------------------------------------
# The queue.
def argument(line, name):
    return re.search(r"\b%s=([^,)]+)" % name, line).group(1)


def test_unweighted_calls_queue_what_they_queued(tmp_path, monkeypatch):
    """Without a weighting compute_kdistribution queues, call for call and argument for argument,
    what it queued before the weighting existed, and never reaches the new entry."""
    from pylbl_amd import spectroscopy as module
    monkeypatch.setattr(module, "_XARRAY", [None])
    golden = json.loads(
        (ROOT / "tests" / "golden" / "kdistribution_unweighted_queue.json").read_text())
    got = wc.unweighted_queues(tmp_path)
    assert set(golden) == set(got) == set(wc.unweighted_calls())
    for name, log in golden.items():
        assert got[name] == log, name
        assert any(line.startswith("band_distribution(") for line in log), name
        assert not any(line.startswith(("band_distribution_weighted", "solar_spectrum"))
                       for line in log), name
    with wc.recorded(tmp_path) as (spec, engine):
        _, result = wc.queue_of(spec, engine, None, dict(band_edges=[20., 30., 60.]))
        assert "weighting" not in result


@pytest.mark.parametrize("weighting", ["planck", "array"])
def test_a_weighted_call_queues_one_entry_per_run(tmp_path, monkeypatch, weighting):
    from pylbl_amd import spectroscopy as module
    monkeypatch.setattr(module, "_XARRAY", [None])
    every = paths.KDISTRIBUTION_QUANTITIES + WEIGHTED
    with wc.recorded(tmp_path) as (spec, engine):
        weights = np.linspace(1., 2., spec.grid.size)
        keywords = dict(band_edges=[20., 30., 45., 60.], g_edges=4, quantities=every,
                        weighting="planck" if weighting == "planck" else weights)
        # Five blocks per level: 30 rows hold the six levels, 29 five of them.
        for limit, runs in ((None, 1), (30, 1), (29, 2), (10, 3), (5, 6)):
            log, result = wc.queue_of(spec, engine, limit, keywords)
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            calls = [line for line in log if line.startswith("band_distribution_weighted(")]
            assert len(calls) == runs
            assert not any(line.startswith("band_distribution(") for line in log)
            uploads = [line for line in log if line.startswith("solar_spectrum(")]
            assert len(uploads) == (0 if weighting == "planck" else 1)
            for line in calls:
                blocks = [argument(line, name).split("[")[0] for name in
                          ("values", "scratch", "index_rows", "index_scratch", "weight_rows",
                           "weighted_rows", "weight_sums", "weighted_sums", "means", "quantiles")]
                assert len(set(blocks)) == 10, line
                assert argument(line, "asynchronous") == "True"
                if weighting == "planck":
                    assert argument(line, "weight_row") == "None"
                    assert argument(line, "row_temperature") != "None"
                else:
                    assert argument(line, "row_temperature") == "None"
                    assert argument(line, "weight_row") == argument(uploads[0], "row")
                    assert argument(uploads[0], "scale") == "1.0"
                    assert log.index(uploads[0]) < log.index(calls[0])
            assert result["weighting"] == weighting
            assert result["weight_g_fraction"].shape == SHAPE + (3, 4)
            assert result["absorption_g_weighted_mean"].shape == SHAPE + (3, 4)
            assert result["sorted_column"].shape == SHAPE + (160,)
            assert result["sorted_column"].dtype == np.int32
        # Only what is asked for is made: no rows of weights for the permutation alone.
        log, result = wc.queue_of(spec, engine, None, dict(
            band_edges=[20., 60.], quantities="sorted_column", weighting=keywords["weighting"]))
        call, = [line for line in log if line.startswith("band_distribution_weighted(")]
        for name in ("weight_rows", "weighted_rows", "weight_sums", "weighted_sums", "means",
                     "quantiles", "interval_start"):
            assert argument(call, name) == "None", name
        assert set(result) >= {"sorted_column", "wavenumber", "g", "weighting"}
        assert "sorted_absorption" not in result


# ---------------------------------------------------------------------------------------------
# The fractions and weighted means formed on the host from the device's sums.
def dataset_of(spec, values, weights, quantities, band_edges, g_edges, monkeypatch):
    """paths._create_kdistribution_dataset fed with the mirror's sums of `values` [levels, grid]
    (float64 roundings of the long-double sums: what the device's sums are within MEAN_BOUND)."""
    from pylbl_amd import spectroscopy as module
    monkeypatch.setattr(module, "_XARRAY", [None])
    rq = request(spec, quantities, weights, band_edges=band_edges, g_edges=g_edges)
    intervals = rq.interval_starts.ravel()
    order, ordered = wc.sorted_rows(values, rq.starts)
    w, wk = wc.gathered(order, ordered, rq.starts, weights, fill=0.)
    bands, q = rq.starts.size - 1, rq.g_edges.size - 1
    mean = np.full((values.shape[0], bands*(q + 1)), np.nan)
    for b in range(bands):
        part = ordered[:, rq.starts[b]:rq.starts[b + 1]]
        mean[:, b*(q + 1):b*(q + 1) + q] = cases.interval_mean_rows(part, rq.g_edges)[0]
    pairs = np.zeros((values.shape[0], 2*((GRID.size + 1)//2)), dtype=np.int32)
    pairs[:, :GRID.size] = order
    device = {paths._WEIGHT_SUMS: wc.interval_sums(w, intervals)[0].astype(F64),
              paths._WEIGHTED_SUMS: wc.interval_sums(wk, intervals)[0].astype(F64),
              "absorption_g_mean": mean[:, :-1], "sorted_column": pairs.view(F64)}
    return paths._create_kdistribution_dataset(spec, device, rq), rq, order


def test_fractions_sum_to_one_and_constant_weights_give_the_arithmetic_mean(monkeypatch):
    spec = spectroscopy()
    rng = np.random.default_rng(9)
    values = rng.lognormal(-8., 3., (6, GRID.size))
    every = ("absorption_g_mean",) + WEIGHTED
    edges = [1000., 1003., 1003.001, 1003.002, 1010.]       # 300, 0 (or 1), ... points
    for g_edges in (1, 5, 16):
        for weights in (np.full(GRID.size, 0.75), wc.planck_weights(F64, GRID, [250.])[0],
                        rng.random(GRID.size)):
            out, rq, order = dataset_of(spec, values, weights, every, edges, g_edges, monkeypatch)
            points = np.diff(rq.starts)
            assert np.any(points == 0) and np.any(points > 4096//8)
            fraction = out["weight_g_fraction"]
            assert fraction.shape == SHAPE + (4, rq.g_edges.size - 1)
            filled = points > 0
            total = np.sum(fraction[..., filled, :].astype(LD), axis=-1)
            assert np.all(np.abs(total - 1) <= LD(1e-12)), g_edges
            assert np.all(np.isnan(fraction[..., ~filled, :]))
            empty = np.diff(rq.interval_starts, axis=1) == 0
            assert np.all(fraction[..., filled[:, None] & empty] == 0.)
            assert np.all(np.isnan(out["absorption_g_weighted_mean"][..., empty]))
            assert out["weighting"] == "array"
            column = out["sorted_column"].reshape(6, GRID.size)
            inside = (np.arange(GRID.size) >= rq.starts[0]) & (np.arange(GRID.size) < rq.starts[-1])
            assert column.dtype == np.int32 and np.array_equal(column[:, inside], order[:, inside])
            assert np.all(column[:, ~inside] == -1)
            if np.all(weights == weights[0]):
                # W is constant: swk/sw is the arithmetic mean of the interval.
                mean = out["absorption_g_mean"]
                weighted = out["absorption_g_weighted_mean"]
                assert np.array_equal(np.isnan(mean), np.isnan(weighted))
                ok = ~np.isnan(mean)
                error = np.abs(weighted[ok].astype(LD) - mean[ok].astype(LD))
                assert np.all(error <= cases.MEAN_BOUND*np.abs(mean[ok]))


def test_a_band_of_zero_weight_has_no_fractions(monkeypatch):
    spec = spectroscopy()
    values = np.random.default_rng(2).lognormal(-8., 3., (6, GRID.size))
    weights = np.where(GRID < 1005., 0., 1.)
    out, rq, _ = dataset_of(spec, values, weights, WEIGHTED, (1000., 1005., 1010.), 4,
                            monkeypatch)
    assert np.all(np.isnan(out["weight_g_fraction"][..., 0, :]))
    assert np.all(np.isnan(out["absorption_g_weighted_mean"][..., 0, :]))
    assert np.all(np.isfinite(out["weight_g_fraction"][..., 1, :]))
    assert np.all(np.isfinite(out["absorption_g_weighted_mean"][..., 1, :]))
