"""Spectroscopy.compute_kdistribution with a weighting on the GPU against plain numpy applied to
compute_absorption("total") of the same Spectroscopy: pi is the stable argsort of the integer keys
exactly, the sorted block and the unweighted quantities keep their bits, and the Planck fractions
and weighted means agree with long-double sums through the mirror's pi.

Bounds, none from the code under test.  The device holds each sum to MEAN_BOUND = 1e-12 x the sum
of the magnitudes of its terms (tests/test_gpu_band_sort_pairs.py), and B(nu, T) in float64 lies
within 1e-14 of the long-double one.  A fraction sw_q/sum_q sw_q of weights >= 0 is then within
(1e-12 + 1e-14) of the numerator + the same of the denominator + the roundings of the host's sum
and quotient, (Q + 2) 1.1e-16: 2.5e-12 x the fraction.  A weighted mean swk_q/sw_q is within
2.5e-12 x (sum |WK|)/sw_q.  Runs of one level, forced by device_output_limit, give the bits of one
run, and a call without a weighting gives the same bits before and after weighted calls on the
same object."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from tests import kdistribution_cases as cases
from tests import kdistribution_weighted_cases as wc

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
GASES = ("H2O", "CO2", "O3")
SHAPE = (2, 2)
GRID = np.arange(600., 700., 0.005)             # 20 000 points
# Bands of 0, 1 901, 0, 13 100 (four chunks: two merge passes), 3 000 and 1 999 points.
EDGES = np.array([590., 599.5, 609.5, 609.502, 675., 690., 700.5])
PLAIN = ("absorption_g_mean", "absorption_g_quantile", "sorted_absorption")
WEIGHTED = ("weight_g_fraction", "absorption_g_weighted_mean", "sorted_column")
Q = 8
BOUND = LD(2.5e-12)
_CACHE = {}


def spectroscopy(**keywords):
    if "tables" not in _CACHE:
        _CACHE["tables"] = [synthetic.line_table(name, 576., 724., num_lines=2000, seed=80 + i)
                            for i, name in enumerate(GASES)]
    full = synthetic.standard_atmosphere(int(np.prod(SHAPE)))
    atmosphere = synthetic.Atmos(p=full.p.reshape(SHAPE), t=full.t.reshape(SHAPE),
                                 vmr={k: full.vmr[k].reshape(SHAPE) for k in GASES})
    spec = Spectroscopy(atmosphere, GRID, MemoryDatabase(_CACHE["tables"]))
    for name, value in keywords.items():
        setattr(spec, name, value)
    return spec


def mirror():
    """(starts, pi [levels, grid], sorted rows) of compute_absorption("total"), formed once and
    left unchanged."""
    if "mirror" not in _CACHE:
        beta = np.array(spectroscopy().compute_absorption("total")["absorption"])
        starts = np.searchsorted(GRID, EDGES, side="left")
        order, ordered = wc.sorted_rows(beta.reshape(-1, GRID.size), starts, fill=-1)
        for array in (order, ordered):
            array.setflags(write=False)
        _CACHE["mirror"] = (starts, order, ordered)
    return _CACHE["mirror"]


def check_against_numpy(out, weights, name):
    """out's weighted quantities against the long-double sums of `weights` [levels, grid] (long
    double) carried through the mirror's pi."""
    starts, order, ordered = mirror()
    levels, bands = order.shape[0], starts.size - 1
    points = np.diff(starts)
    assert points.tolist() == [0, 1901, 0, 13100, 3000, 1999]
    assert out["weighting"] == name if isinstance(out, dict) else out.attrs["weighting"] == name
    column = np.asarray(out["sorted_column"]).reshape(levels, GRID.size)
    assert column.dtype == np.int32 and np.array_equal(column, order)
    in_band = order[0] >= 0
    got = np.asarray(out["sorted_absorption"]).reshape(levels, GRID.size)
    assert cases.same_bits(got[:, in_band], ordered[:, in_band])
    assert np.all(np.isnan(got[:, ~in_band]))
    w = np.zeros(order.shape, dtype=LD)
    for b in range(bands):
        a, e = int(starts[b]), int(starts[b + 1])
        w[:, a:e] = np.take_along_axis(weights[:, a:e], order[:, a:e].astype(np.int64), axis=1)
    wk = w*np.where(in_band, ordered, 0.).astype(LD)
    intervals = wc.flat_intervals(starts, cases.gauss_edges(Q))
    sw = wc.per_band(wc.interval_sums(w, intervals)[0], bands, Q)
    swk, size = (wc.per_band(x, bands, Q) for x in wc.interval_sums(wk, intervals))
    fraction = np.asarray(out["weight_g_fraction"]).reshape(levels, bands, Q)
    weighted = np.asarray(out["absorption_g_weighted_mean"]).reshape(levels, bands, Q)
    filled = points > 0
    assert np.all(np.isnan(fraction[:, ~filled])) and np.all(np.isnan(weighted[:, ~filled]))
    exact = sw[:, filled]/np.sum(sw[:, filled], axis=-1, keepdims=True)
    error = np.abs(fraction[:, filled].astype(LD) - exact)
    with np.errstate(invalid="ignore", divide="ignore"):
        print("%s: worst fraction error / bound %.3g" % (
            name, float(np.nanmax(error/(BOUND*exact)))))
    assert np.all(error <= BOUND*exact)
    assert np.all(np.abs(np.sum(fraction[:, filled].astype(LD), axis=-1) - 1) <= LD(1e-12))
    assert np.all(sw[:, filled] > 0)
    exact = swk[:, filled]/sw[:, filled]
    allowed = BOUND*size[:, filled]/sw[:, filled]
    error = np.abs(weighted[:, filled].astype(LD) - exact)
    print("%s: worst weighted-mean error / bound %.3g" % (name, float(np.max(error/allowed))))
    assert np.all(error <= allowed)
    # a mean of the interval's k, whatever the weights: between its least and greatest value
    for b in np.flatnonzero(filled):
        bounds = starts[b] + cases.interval_bounds(points[b], cases.gauss_edges(Q))
        for q in range(Q):
            part = ordered[:, bounds[q]:bounds[q + 1]]
            slack = 1e-12*np.abs(part).max(axis=1)
            assert np.all(weighted[:, b, q] >= part[:, 0] - slack)
            assert np.all(weighted[:, b, q] <= part[:, -1] + slack)


def test_unweighted_bits_before_and_after_weighted_calls_and_planck_default():
    spec = spectroscopy()
    before = spec.compute_kdistribution(EDGES, Q, quantities=PLAIN)
    out = spec.compute_kdistribution(EDGES, Q, quantities=PLAIN + WEIGHTED, weighting="planck")
    after = spec.compute_kdistribution(EDGES, Q, quantities=PLAIN)
    for name in PLAIN:
        assert cases.same_bits(np.asarray(after[name]), np.asarray(before[name])), name
        # ... and the weighted call's own: the pair sort leaves the plain sort's values
        assert cases.same_bits(np.asarray(out[name]), np.asarray(before[name])), name
    assert "weighting" not in before and "weighting" not in getattr(before, "attrs", {})
    for name in WEIGHTED:
        assert name not in before
    temperature = np.asarray(spec.atmosphere.temperature, dtype=F64).ravel()
    check_against_numpy(out, wc.planck_weights(LD, GRID, temperature), "planck")
    _CACHE["planck"] = {name: np.array(out[name]) for name in PLAIN + WEIGHTED}


@pytest.mark.parametrize("temperature", [250., "array"])
def test_planck_at_a_given_temperature(temperature):
    if isinstance(temperature, str):
        temperature = np.array([[180., 288.], [320., 210.]])
    out = spectroscopy().compute_kdistribution(
        EDGES, Q, quantities=("sorted_absorption",) + WEIGHTED, weighting="planck",
        weighting_temperature=temperature)
    flat = np.broadcast_to(np.asarray(temperature, dtype=F64), SHAPE).ravel()
    check_against_numpy(out, wc.planck_weights(LD, GRID, flat), "planck")


def test_an_array_of_weights():
    """A solar-like spectrum with a stretch of zeros: the same weights at every level."""
    rng = np.random.default_rng(31)
    weights = wc.planck_weights(F64, GRID, [5772.])[0]*6.794e-5*rng.uniform(0.6, 1., GRID.size)
    weights[4000:4100] = 0.
    out = spectroscopy().compute_kdistribution(
        EDGES, Q, quantities=("sorted_absorption",) + WEIGHTED, weighting=weights)
    check_against_numpy(out, np.broadcast_to(weights.astype(LD), (4, GRID.size)), "array")
    # Constant weights: the weighted mean is the arithmetic one.
    out = spectroscopy().compute_kdistribution(
        EDGES, Q, quantities=("absorption_g_mean", "absorption_g_weighted_mean"),
        weighting=np.full(GRID.size, 0.75))
    mean = np.asarray(out["absorption_g_mean"])
    weighted = np.asarray(out["absorption_g_weighted_mean"])
    ok = ~np.isnan(mean)
    assert np.array_equal(np.isnan(weighted), ~ok) and np.any(ok)
    starts, order, ordered = mirror()
    for b in range(starts.size - 1):
        part = ordered[:, starts[b]:starts[b + 1]]
        if part.shape[1] == 0:
            continue
        _, magnitude = cases.interval_mean_rows(part, cases.gauss_edges(Q))
        error = np.abs(weighted.reshape(4, -1, Q)[:, b].astype(LD) -
                       mean.reshape(4, -1, Q)[:, b].astype(LD))
        # each of swk, sw and the arithmetic mean is within MEAN_BOUND of its exact value
        held = ~np.isnan(magnitude)
        assert np.all(error[held] <= 3*cases.MEAN_BOUND*magnitude[held])


def test_runs_of_one_level_give_the_same_bits():
    """A device_output_limit that holds the five blocks of one level only."""
    if "planck" not in _CACHE:
        out = spectroscopy().compute_kdistribution(EDGES, Q, quantities=PLAIN + WEIGHTED,
                                                   weighting="planck")
        _CACHE["planck"] = {name: np.array(out[name]) for name in PLAIN + WEIGHTED}
    whole = _CACHE["planck"]
    cut = spectroscopy(device_output_limit=5*GRID.size*8 + 64).compute_kdistribution(
        EDGES, Q, quantities=PLAIN + WEIGHTED, weighting="planck")
    for name in PLAIN + WEIGHTED:
        got, expected = np.asarray(cut[name]), whole[name]
        if name == "sorted_column":
            assert np.array_equal(got, expected), name
        else:
            assert cases.same_bits(got, expected), name
