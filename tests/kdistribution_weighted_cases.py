"""What the tests of the weighted k-distributions share (lbl_band_distribution_weighted,
Spectroscopy.compute_kdistribution with weighting=): the numpy mirror of the contract -- integer
keys, numpy.argsort(kind="stable"), one product per column, long-double sums -- the value kinds on
which ties decide the permutation, and a stand-in engine that writes down what a call queues.
The keys, the plain oracles and the merge generators are tests/kdistribution_cases.py's."""
import contextlib

import numpy as np

from tests import kdistribution_cases as cases
from tests import solar_cases as solar
from tests import surface_cases as surface
from tests.sweep_cases import planck

F64, LD, U64 = np.float64, np.longdouble, np.uint64
MEAN_BOUND = cases.MEAN_BOUND
SENTINEL = cases.SENTINEL
INDEX_SENTINEL = -777
# The NaN whose key is the pad key of a short chunk (kSortMaxKey): it must still sort in front
# of the padding.
MAX_KEY_NAN = np.array([0x7FFFFFFFFFFFFFFF], dtype=U64).view(F64)[0]
NANS = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0x7FF8000000000001],
                dtype=U64).view(F64)
PLANCK_TEMPERATURES = (180., 288., 320.)

# Band lengths: around the 8-key minimum of the network and a wavefront, the chunk (no and one
# merge pass), an unpaired run with an odd and an even number of passes, a partner run one short
# of, exactly and one over a tile, and one band of three passes and a value.
LENGTHS = [1, 7, 8, 9, 127, 128, 129, 130, 4095, 4096, 4097, 2*4096 + 5, 3*4096 + 1, 6143, 6144,
           6145, 2**15 + 1]
VALUE_KINDS = ("equal", "two values", "plateau", "zero plateau", "signed zeros", "nans",
               "infinities", "random")


def values_of(kind, n, rng):
    """n float64 values of a kind of VALUE_KINDS: many equal keys, in every one but "random"."""
    if kind == "equal":
        return np.full(n, 3.25e-7)
    if kind == "two values":
        return np.where(rng.random(n) < 0.5, 1.5e-3, 2.5e-9)
    if kind == "plateau":
        return cases.merge_values_of("plateau", n, rng)
    if kind == "zero plateau":
        return cases.merge_values_of("plateau", n, rng, signed_zeros=True)
    if kind == "signed zeros":
        return rng.choice(np.array([0., -0., 0., -0., 1e-300, -1e-300]), n)
    if kind == "nans":
        # Few real values, the NaNs of several payloads among them: a short chunk of these holds
        # the pad key next to its padding.
        out = rng.choice(np.concatenate([NANS, [MAX_KEY_NAN, MAX_KEY_NAN, 1., -1., 0.]]), n)
        out[rng.integers(n)] = MAX_KEY_NAN
        return np.ascontiguousarray(out, dtype=F64)
    if kind == "infinities":
        return rng.choice(np.array([np.inf, -np.inf, np.inf, 0., 2.5, -2.5]), n)
    assert kind == "random"
    return rng.lognormal(-8., 3., n)


def stable_order(values):
    """pi of one band: numpy.argsort of the integer keys, stable (int32 offsets)."""
    return np.argsort(cases.keys(values), kind="stable").astype(np.int32)


def sorted_rows(values, starts, fill=INDEX_SENTINEL):
    """(pi [rows, columns] int32 with `fill` outside the bands, the sorted rows) of every band of
    every row."""
    values = np.asarray(values, dtype=F64)
    order = np.full(values.shape, fill, dtype=np.int32)
    ordered = values.copy()
    for r in range(values.shape[0]):
        for b in range(len(starts) - 1):
            a, e = int(starts[b]), int(starts[b + 1])
            order[r, a:e] = stable_order(values[r, a:e])
            ordered[r, a:e] = values[r, a:e][order[r, a:e]]
    return order, ordered


def gathered(order, ordered, starts, weights, fill=SENTINEL):
    """(W, WK) [rows, columns] in float64: W_i = w_pi(i) and WK_i = W_i*k_i, one product; `fill`
    outside the bands.  weights: [columns], or [rows, columns] (one row of weights per row)."""
    weights = np.broadcast_to(np.asarray(weights, dtype=F64), ordered.shape)
    w = np.full(ordered.shape, fill)
    wk = np.full(ordered.shape, fill)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(len(starts) - 1):
            a, e = int(starts[b]), int(starts[b + 1])
            w[:, a:e] = np.take_along_axis(weights[:, a:e], order[:, a:e].astype(np.int64), axis=1)
            wk[:, a:e] = w[:, a:e]*ordered[:, a:e]
    return w, wk


def interval_sums(rows, interval_starts):
    """(long-double sum, long-double sum of magnitudes) [rows, intervals] of the columns
    [interval_starts[q], interval_starts[q + 1])."""
    rows = np.asarray(rows)
    count = len(interval_starts) - 1
    total = np.zeros((rows.shape[0], count), dtype=LD)
    size = np.zeros((rows.shape[0], count), dtype=LD)
    for q in range(count):
        part = rows[:, int(interval_starts[q]):int(interval_starts[q + 1])].astype(LD)
        total[:, q] = np.sum(part, axis=1)
        size[:, q] = np.sum(np.abs(part), axis=1)
    return total, size


def planck_weights(kind, grid, temperatures):
    """[rows, columns]: B(nu, T_row) in `kind` (float64: the stated order; long double: the
    reference)."""
    return planck(kind, np.asarray(grid)[None, :], np.asarray(temperatures)[:, None])


def flat_intervals(starts, g_edges):
    """The device's flat interval list of bands `starts`: every band's Q + 1 starts in a row."""
    return np.concatenate([starts[b] + cases.interval_bounds(n, g_edges)
                           for b, n in enumerate(np.diff(starts))]).astype(np.int64)


def per_band(flat, bands, q):
    """[rows, bands, Q] of the device's [rows, bands (Q + 1) - 1]: the gaps dropped."""
    flat = np.asarray(flat)
    padded = np.zeros((flat.shape[0], bands*(q + 1)), dtype=flat.dtype)
    padded[:, :-1] = flat
    return padded.reshape(flat.shape[0], bands, q + 1)[:, :, :q]


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class KDistributionRecorder(solar.SolarRecorder):
    """tests/solar_cases.py's engine with the two k-distribution calls."""
    def band_distribution(self, values, columns, band_start, **keywords):
        self.record("band_distribution", values=values, columns=columns,
                    band_start=np.asarray(band_start), **self._described(keywords))

    def band_distribution_weighted(self, values, columns, band_start, index_rows, **keywords):
        self.record("band_distribution_weighted", values=values, columns=columns,
                    band_start=np.asarray(band_start), index_rows=index_rows,
                    **self._described(keywords))


@contextlib.contextmanager
def recorded(directory):
    """surface_cases.recorded with a KDistributionRecorder."""
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = KDistributionRecorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before


def unweighted_calls():
    """{name: (device_output_limit in rows, keywords)}: calls of compute_kdistribution without a
    weighting -- what tests/golden/kdistribution_unweighted_queue.json records."""
    every = ("absorption_g_mean", "absorption_g_quantile", "sorted_absorption")
    return {
        "default": (None, dict(band_edges=[20., 30., 45., 60.])),
        "every quantity": (None, dict(band_edges=[20., 30., 45., 60.], g_edges=4,
                                      g_points=[0., 0.5, 1.], quantities=every)),
        "runs of two levels": (4, dict(band_edges=[25., 55.], g_edges=3, quantities=every,
                                       range_policy="skip")),
        "one level a run, quantiles": (2, dict(band_edges=[20., 20.1, 60.], g_edges=[0., 0.4, 1.],
                                               quantities="absorption_g_quantile",
                                               remove_pedestal=False)),
    }


def queue_of(spec, engine, limit_rows, keywords):
    """The log of spec.compute_kdistribution(**keywords) with device_output_limit = limit_rows
    rows, and the result."""
    spec.device_output_limit = (8 << 30) if limit_rows is None else limit_rows*surface.ROW_BYTES
    engine.begin()
    result = spec.compute_kdistribution(**keywords)
    return list(engine.log), result


def unweighted_queues(directory):
    with recorded(directory) as (spec, engine):
        return {name: queue_of(spec, engine, limit, keywords)[0]
                for name, (limit, keywords) in unweighted_calls().items()}
