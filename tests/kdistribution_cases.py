"""Cases and plain-numpy oracles of the k-distribution tests (lbl_band_distribution,
Spectroscopy.compute_kdistribution): nothing here is imported from pylbl_amd.

The order: with u the 64 bits of a value, key = u ^ 2^63 for a clear sign bit, ~u for a set one,
keys compared as unsigned integers.  The oracle sorts the keys with numpy.sort and maps them back,
so the expected rows are unique bit for bit."""
import numpy as np

F64, LD, U64 = np.float64, np.longdouble, np.uint64
SIGN = U64(1) << U64(63)
SENTINEL = -12345.678
MEAN_BOUND = LD(1e-12)      # x mean |k|: the bound the project holds its band means to

# Segment lengths: every N in 1..130, then around the powers of two and 3 2^k + 5 for k = 7..15.
SMALL_LENGTHS = list(range(1, 131))
LARGE_LENGTHS = [n for k in range(7, 16) for n in (2**k - 1, 2**k, 2**k + 1, 3*2**k + 5)]
# 3 2^15 + 5 values are only four chunks of 32 768 (two passes): one longer segment, nine such
# chunks, so that every chunk size of CHUNKS meets four passes and a run without a partner.
LARGE_LENGTHS.append(2**18 + 1)
LENGTHS = SMALL_LENGTHS + LARGE_LENGTHS
VALUE_KINDS = ("random", "equal", "sorted", "reversed", "two values", "mix")
FINITE_KINDS = VALUE_KINDS[:5]
HOST_LENGTHS = (0, 1, 2, 3, 16, 17, 10001)
CHUNKS = [2**k for k in range(7, 16)]       # every power-of-two chunk from 128 to 32 768


def keys(values):
    u = np.ascontiguousarray(values, dtype=F64).view(U64)
    return np.where(u & SIGN != 0, ~u, u ^ SIGN)


def from_keys(k):
    k = np.ascontiguousarray(k, dtype=U64)
    return np.where(k & SIGN != 0, k ^ SIGN, ~k).astype(U64).view(F64)


def key_sort(values):
    """A 1-d array sorted ascending by the integer key: the same bits, permuted."""
    return from_keys(np.sort(keys(values)))


def sort_bands(rows, starts):
    """[rows, columns] with every band of every row sorted by the key; other columns as they are."""
    out = np.array(rows, dtype=F64)
    for r in range(out.shape[0]):
        for b in range(len(starts) - 1):
            out[r, starts[b]:starts[b + 1]] = key_sort(out[r, starts[b]:starts[b + 1]])
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F64), np.ascontiguousarray(b, dtype=F64)
    return a.shape == b.shape and np.array_equal(a.view(U64), b.view(U64))


def same_bits_or_nan(got, expected):
    """The same bits wherever the expected value is a number or an infinity, NaN where it is NaN
    (the payload of a NaN that arithmetic makes, inf - inf or 0*inf, is the machine's own)."""
    got, expected = np.asarray(got, dtype=F64), np.asarray(expected, dtype=F64)
    nan = np.isnan(expected)
    return got.shape == expected.shape and np.array_equal(np.isnan(got), nan) and \
        same_bits(got[~nan], expected[~nan])


def gauss_edges(count):
    _, w = np.polynomial.legendre.leggauss(count)
    edges = np.concatenate([[0.], np.cumsum(w/2.)])
    edges[-1] = 1.
    return edges


def gauss_points(count):
    x, _ = np.polynomial.legendre.leggauss(count)
    return (x + 1.)/2.


def interval_bounds(n, g_edges):
    """[Q + 1] sample bounds of a band of n points, one edge at a time: ceil(G n) in fp64."""
    return np.array([int(np.ceil(F64(g)*F64(n))) for g in g_edges], dtype=np.int64)


def quantile_index(n, g):
    """(i, f) of one g point of a band of n >= 1 points, the issue's statement."""
    x = min(max(F64(g)*F64(n) - F64(0.5), F64(0.)), F64(n - 1))
    i = int(np.floor(x))
    return i, F64(x) - F64(i)


def quantiles(sorted_band, g_points):
    """k_i + f*(k_min(i+1, N-1) - k_i) at every g point; NaN for an empty band."""
    n = sorted_band.size
    out = np.full(len(g_points), np.nan)
    if n == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        for p, g in enumerate(g_points):
            i, f = quantile_index(n, g)
            k = sorted_band[i]
            out[p] = k + f*(sorted_band[min(i + 1, n - 1)] - k)
    return out


def interval_means(sorted_band, g_edges):
    """(long-double mean, long-double mean of |k|) per interval; NaN for one without samples."""
    bounds = interval_bounds(sorted_band.size, g_edges)
    mean = np.full(len(g_edges) - 1, np.nan, dtype=LD)
    magnitude = np.full(len(g_edges) - 1, np.nan, dtype=LD)
    for q in range(len(g_edges) - 1):
        part = sorted_band[bounds[q]:bounds[q + 1]].astype(LD)
        if part.size:
            mean[q] = np.sum(part)/LD(part.size)
            magnitude[q] = np.sum(np.abs(part))/LD(part.size)
    return mean, magnitude


def merge_passes(n, chunk):
    """Merge passes a segment of n values takes after chunks of `chunk` are sorted."""
    runs, passes = -(-n//chunk), 0
    while runs > 1:
        runs, passes = -(-runs//2), passes + 1
    return passes


def unpaired_passes(n, chunk):
    """How many of those passes meet an odd number (> 1) of runs: a last run without a partner."""
    runs, found = -(-n//chunk), 0
    while runs > 1:
        found += runs % 2
        runs = -(-runs//2)
    return found


def values_of(kind, n, rng):
    """n float64 values of a kind."""
    if kind == "random":
        return rng.lognormal(-8., 3., n)
    if kind == "equal":
        return np.full(n, 3.25e-7)
    if kind == "sorted":
        return np.sort(rng.lognormal(-8., 3., n))
    if kind == "reversed":
        return np.sort(rng.lognormal(-8., 3., n))[::-1].copy()
    if kind == "two values":
        return np.where(rng.random(n) < 0.5, 1.5e-3, 2.5e-9)
    assert kind == "mix"
    pool = np.array([0., -0., np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, 1e-310, -1e-310, -1., 1.,
                     -3.5e7, 3.5e7, 1e-30, 1e-30, 7.25, 7.25, 7.25], dtype=F64)
    nan = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF],
                   dtype=U64).view(F64)
    out = rng.choice(np.concatenate([pool, nan, rng.normal(0., 1., 8)]), n)
    return np.ascontiguousarray(out, dtype=F64)


def packed_starts(lengths):
    """Band starts of the lengths side by side in one row, an empty band after every third and
    unbanded columns at both ends: (starts [B + 1], columns, indices of the real bands).  Every
    second gap between bands is closed by a band of no columns, so the starts stay one list."""
    starts, at, real = [5], 5, []
    for i, n in enumerate(lengths):
        real.append(len(starts) - 1)
        at += n
        starts.append(at)
        if i % 3 == 2:
            starts.append(at)           # an empty band
    return np.array(starts, dtype=np.int64), at + 7, real


# ---------------------------------------------------------------------------------------------
# Beyond the lengths above: the run arithmetic of the 4096 chunk and 2048 tile (band_sort.h) --
# 4096 + 2047 / 2048 / 2049 (a partner run one short of, exactly and one over a tile), three full
# runs, three runs with the last 7 short, 5 1/2 runs and a value (an unpaired run of 6145 that the
# third pass merges) and two runs and a tile.
EXTRA_LENGTHS = [6143, 6144, 6145, 12288, 12281, 22529, 2*4096 + 2048]
# Inputs for merge path's splits (merge_values_of): the kinds the tuple above does not hold.
MERGE_KINDS = ("interleaved", "plateau", "blocks")
SORT_CHUNK, MERGE_TILE = 4096, 2048


def merge_pass_tiles(n, chunk=SORT_CHUNK, tile=MERGE_TILE):
    """[(run, [(na, nb, d0, count) per tile])] per merge pass of a segment of n values, from the
    comment at the top of band_sort.h: pass p merges neighbouring runs of chunk*2^p values; the
    tile of outputs [offset, offset + tile) lies in the pair of runs that starts at the multiple
    of 2*run below offset, a = the pair's first na values, b its next nb (0: a run without a
    partner, copied through), d0 the tile's offset in the pair and count its outputs."""
    passes = []
    for p in range(merge_passes(n, chunk)):
        run, tiles = chunk << p, []
        for offset in range(0, n, tile):
            pair = offset//(2*run)*(2*run)
            left = n - pair
            na = min(left, run)
            nb = min(left - na, run)
            d0 = offset - pair
            tiles.append((na, nb, d0, min(na + nb - d0, tile)))
        passes.append((run, tiles))
    return passes


def merge_tiles(n, chunk=SORT_CHUNK, tile=MERGE_TILE):
    """(na, nb, d0, count) of every tile of every merge pass of a segment of n values."""
    for _, tiles in merge_pass_tiles(n, chunk, tile):
        for one in tiles:
            yield one


def ascending(n, rng, low=1e-9):
    """n strictly ascending positive values: no two share their bits."""
    return low*np.cumsum(0.1 + rng.random(n))


def plateau_bounds(n):
    """[lo, hi) of the plateau in the sorted order of n values: [0.4 n, 0.6 n) in integers."""
    return (2*n)//5, (3*n)//5


def merge_values_of(kind, n, rng, signed_zeros=False, chunk=SORT_CHUNK):
    """n float64 values of a kind of MERGE_KINDS, arranged by blocks of `chunk` values (the runs
    after the chunk sort); the order inside a block is random.
    "interleaved": every pair of blocks (2j, 2j + 1) holds a random share of n strictly ascending
        values, dealt alternately: with lb the length of block 2j + 1, the pair's ranks 0, 2, ...,
        2 lb - 2 and everything from 2 lb on go to block 2j, the ranks 1, 3, ..., 2 lb - 1 to
        block 2j + 1 -- every split of the first pass lands inside both runs.
    "plateau": ascending values with one plateau of equal bits at [0.4 n, 0.6 n) of the sorted
        order (plateau_bounds), half of its copies in block 0 and half in block 1 (all in block 0
        while n <= chunk), everything else anywhere.  signed_zeros: the plateau is zero -- below
        it negatives, above it positives -- one half of its copies -0.0 and the other +0.0,
        scattered at random over both blocks.
    "blocks": block i holds the values that n strictly ascending ones have at the places of block
        i counted from the end: every value of a block is greater than every value of each later
        block, so every split of every pass lies at the end of a run."""
    assert kind in MERGE_KINDS and n >= 1
    bounds = list(range(0, n, chunk)) + [n]
    out = np.empty(n, dtype=F64)
    if kind == "interleaved":
        values = ascending(n, rng)
        order = rng.permutation(n)
        for a in range(0, len(bounds) - 1, 2):
            begin, middle = bounds[a], bounds[a + 1]
            end = bounds[a + 2] if a + 2 < len(bounds) else middle
            share = np.sort(values[order[begin:end]])
            lb = end - middle
            out[begin:middle] = rng.permutation(np.concatenate([share[0:2*lb:2], share[2*lb:]]))
            out[middle:end] = rng.permutation(share[1:2*lb:2])
        return out
    if kind == "blocks":
        values = ascending(n, rng)
        for a in range(len(bounds) - 1):
            out[bounds[a]:bounds[a + 1]] = rng.permutation(values[n - bounds[a + 1]:n - bounds[a]])
        return out
    lo, hi = plateau_bounds(n)
    values = ascending(n, rng)
    if signed_zeros and hi > lo:
        values = values - values[lo]
        zeros = np.zeros(hi - lo)
        zeros[:(hi - lo)//2] = -0.
        values[lo:hi] = rng.permutation(zeros)
        assert np.all(values[:lo] < 0.) and np.all(values[hi:] > 0.)
    elif hi > lo:
        values[lo:hi] = values[lo]
    plateau, others = values[lo:hi], rng.permutation(np.concatenate([values[:lo], values[hi:]]))
    size0 = min(n, chunk)
    size1 = min(n, 2*chunk) - size0
    second = min(plateau.size - plateau.size//2, size1)      # the plateau's copies in block 1
    first = plateau.size - second
    assert first <= size0
    cut0, cut1 = size0 - first, size0 - first + size1 - second
    out[:size0] = rng.permutation(np.concatenate([plateau[:first], others[:cut0]]))
    out[size0:size0 + size1] = rng.permutation(np.concatenate([plateau[first:],
                                                               others[cut0:cut1]]))
    out[size0 + size1:] = others[cut1:]
    return out


def sort_band_rows(rows, starts):
    """sort_bands for many rows at once: numpy.sort of the keys along the rows of every band."""
    out = np.array(rows, dtype=F64)
    for b in range(len(starts) - 1):
        a, e = int(starts[b]), int(starts[b + 1])
        if e > a:
            out[:, a:e] = from_keys(np.sort(keys(out[:, a:e]), axis=1))
    return out


def quantile_rows(sorted_rows, g_points):
    """quantiles of one band of many rows [rows, N] at once: the same expression, elementwise."""
    n = sorted_rows.shape[1]
    out = np.full((sorted_rows.shape[0], len(g_points)), np.nan)
    if n == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        for p, g in enumerate(g_points):
            i, f = quantile_index(n, g)
            k = sorted_rows[:, i]
            out[:, p] = k + f*(sorted_rows[:, min(i + 1, n - 1)] - k)
    return out


def interval_mean_rows(sorted_rows, g_edges):
    """interval_means of one band of many rows [rows, N] at once: (mean, mean of |k|), each
    long double [rows, Q]."""
    bounds = interval_bounds(sorted_rows.shape[1], g_edges)
    shape = (sorted_rows.shape[0], len(g_edges) - 1)
    mean, magnitude = np.full(shape, np.nan, dtype=LD), np.full(shape, np.nan, dtype=LD)
    with np.errstate(invalid="ignore"):
        for q in range(len(g_edges) - 1):
            part = sorted_rows[:, bounds[q]:bounds[q + 1]].astype(LD)
            if part.shape[1]:
                mean[:, q] = np.sum(part, axis=1)/LD(part.shape[1])
                magnitude[:, q] = np.sum(np.abs(part), axis=1)/LD(part.shape[1])
    return mean, magnitude
