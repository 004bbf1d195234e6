"""Test helpers for the instrument apply (csrc/instrument.h): a numpy mirror of the sort and
tiling of lbl_instrument_create, the probe channel sets whose windows reach the edges of tiles and
segments, and a reference in extended precision.  Shared by tests/test_instrument_host.py (no GPU)
and tests/test_gpu_instrument_limits.py."""
import math

import numpy as np

from pylbl_amd import Instrument

TILE = 16           # kInstrTile
SEGMENT = 512       # kInstrSegment
ROW_GROUP = 64      # kInstrRowGroup
GRID_Y = 65535      # kPathGridY

# What the probe channel sets must reach (checked by coverage()).
CASES = ("window starts at column 0", "window hi is grid[-1]", "window of 1 column",
         "511 columns from the tile base", "512 columns from the tile base",
         "513 columns from the tile base", "channel spans >= 3 segments",
         "tile with a dropped segment", "valid channels 16k + 1", "invalid channel between valid",
         "duplicated centre")
# Tabulated windows share one width (the offsets are shared), so they cannot be 1 and 513 columns
# wide at once: the tabulated set reaches all the rest.
TABULATED_CASES = tuple(c for c in CASES if c not in (
    "window of 1 column", "511 columns from the tile base", "512 columns from the tile base",
    "513 columns from the tile base"))

PROBE_COLUMNS = 2603        # not a multiple of 8
STEP = 1./64.               # grid values, windows and centres are exact binary fractions
SHAPE_NAMES = ("boxcar", "triangle", "gaussian", "fts", "fts-hamming", "tabulated")
TABLE_OFFSETS = np.array([-4., -1.5, 0., 1., 4.25])
TABLE_RESPONSE = np.array([0., 0.7, 1., 0.4, 0.])


def probe_grid(kind, size=PROBE_COLUMNS, seed=5):
    """600 + (j + u_j)/64: uniform (u = 0) or jittered (u_j a multiple of 2^-10 in [-0.3, 0.3])."""
    j = np.arange(size, dtype=np.float64)
    if kind == "jittered":
        j = j + np.random.default_rng(seed).integers(-300, 301, size)/1024.
    return 600. + j*STEP


def _windows(grid, columns):
    """(lo, hi) of windows over the columns [a, b): a quarter step outside the outer points, but
    lo = grid[0] when a == 0 and hi = grid[-1] when b == len(grid) (still inside the grid)."""
    lo, hi = [], []
    for a, b in columns:
        lo.append(grid[0] if a == 0 else grid[a] - STEP/4.)
        hi.append(grid[-1] if b == grid.size else grid[b - 1] + STEP/4.)
    return np.array(lo), np.array(hi)


def _invalid(grid):
    """Windows of no point, and windows partly below and partly above the grid."""
    n = grid.size
    return (np.array([grid[100] + STEP/4., grid[0] - STEP/4., grid[n - 53] - STEP/4.]),
            np.array([grid[100] + STEP/4. + STEP/16., grid[50] + STEP/4., grid[-1] + STEP/4.]))


def _caller_order(valid, invalid, seed):
    """Valid windows shuffled, the invalid ones put between them."""
    lo, hi = valid
    order = np.random.default_rng(seed).permutation(lo.size)
    lo, hi = list(lo[order]), list(hi[order])
    for i, (a, b) in enumerate(zip(*invalid)):
        at = 1 + i*(len(lo) // 3)
        lo.insert(at, a)
        hi.insert(at, b)
    return np.array(lo), np.array(hi)


def probe_windows(grid):
    """Window columns [a, b) of the 49 = 3*16 + 1 valid channels (sorted; 16 per tile) of the
    probe set of the shapes with per-channel widths, and (lo, hi) of all channels in the caller's
    order, invalid ones included."""
    n = grid.size
    tile0 = [(0, 511), (0, 512), (0, 513), (1, 1400), (2, 3), (4, 300), (4, 300)] + \
        [(5 + i, 60 + 7*i) for i in range(9)]
    # segment 1 of this tile (from its base, column 20) is touched by none of its windows
    tile1 = [(20 + i, 80 + 5*i) for i in range(8)] + [(1200 + i, 1250 + 3*i) for i in range(8)]
    tile2 = [(1210 + 80*i, 1250 + 81*i) for i in range(15)] + [(2400, n)]
    tile3 = [(2500, 2510)]
    columns = tile0 + tile1 + tile2 + tile3
    return columns, _caller_order(_windows(grid, columns), _invalid(grid), seed=11)


def probe_table_windows(grid):
    """As probe_windows for the tabulated shape: every window is TABLE_OFFSETS wide (~528
    columns), so each is given by its first column."""
    n = grid.size
    width = TABLE_OFFSETS[-1] - TABLE_OFFSETS[0]
    firsts = [0, 3, 3] + list(range(4, 16)) + [500]          # tile 0; [500, ~1028): 3 segments
    firsts += list(range(520, 527)) + list(range(2056, 2065))  # tile 1: segment 2 dropped
    firsts += [2065 + i % 5 for i in range(16)]                # tile 2
    lo = np.array([grid[0] if a == 0 else grid[a] - STEP/4. for a in firsts] +
                  [grid[-1] - width])                          # tile 3: hi = grid[-1]
    # a window of this width always holds points: partly below and partly above the grid
    invalid = np.array([grid[0] - STEP/4., grid[n - 100], grid[-1] - width + STEP/4.])
    return _caller_order((lo, lo + width), (invalid, invalid + width), seed=12)


def probe_instrument(name, grid):
    """The probe channel set of one shape on `grid`: windows exactly the designed (lo, hi)."""
    if name == "tabulated":
        lo, hi = probe_table_windows(grid)
        x = Instrument.tabulated(lo - TABLE_OFFSETS[0], TABLE_OFFSETS, TABLE_RESPONSE)
    else:
        _, (lo, hi) = probe_windows(grid)
        center, h = (lo + hi)/2., (hi - lo)/2.
        x = {"boxcar": lambda: Instrument.boxcar(center, hi - lo),
             "triangle": lambda: Instrument.triangle(center, h),
             "gaussian": lambda: Instrument.gaussian(center, h/3., half_width=h),
             "fts": lambda: Instrument.fts(center, 0.8, half_width=h),
             "fts-hamming": lambda: Instrument.fts(center, 0.8, apodization="hamming",
                                                   half_width=h)}[name]()
    got_lo, got_hi = x.window()
    assert np.array_equal(got_lo, lo) and np.array_equal(got_hi, hi)
    return x


def tiling(instrument, grid):
    """numpy mirror of lbl_instrument_create: the windows' columns, which channels are valid, the
    tiles of kInstrTile valid channels in window order, their items (tile, begin, end) -- the
    segments of kInstrSegment columns cut from each tile's first column that some window of the
    tile touches -- and each channel's tile, slot, first item and item count."""
    begin, end = instrument.columns(grid)
    valid = instrument.covered(grid)
    ids = np.flatnonzero(valid)
    order = ids[np.lexsort((end[ids], begin[ids]))]     # stable, like std::stable_sort
    items, tiles = [], []
    tile_of = np.full(len(instrument), -1)
    slot = np.full(len(instrument), -1)
    first_item = np.full(len(instrument), -1)
    n_items = np.zeros(len(instrument), dtype=np.int64)
    for t in range(0, order.size, TILE):
        members = order[t:t + TILE]
        base = int(begin[members[0]])
        union_end = int(end[members].max())
        item_of = {}
        for s in range(-(-(union_end - base) // SEGMENT)):
            b = base + s*SEGMENT
            e = min(b + SEGMENT, union_end)
            if np.any((begin[members] < e) & (end[members] > b)):
                item_of[s] = len(items)
                items.append((t // TILE, b, e))
        tiles.append(dict(base=base, end=union_end, members=members,
                          segments=-(-(union_end - base) // SEGMENT), items=len(item_of)))
        for i, c in enumerate(members):
            tile_of[c], slot[c] = t // TILE, i
            first = (begin[c] - base) // SEGMENT
            last = (end[c] - 1 - base) // SEGMENT
            first_item[c] = item_of[first]
            n_items[c] = last - first + 1
            assert all(s in item_of for s in range(first, last + 1))
            assert [item_of[s] for s in range(first, last + 1)] == \
                list(range(item_of[first], item_of[first] + n_items[c]))
    return dict(begin=begin, end=end, valid=valid, order=order, items=items, tiles=tiles,
                tile=tile_of, slot=slot, first_item=first_item, n_items=n_items)


def launch_chunk(n_items, rows):
    """Rows per launch of lbl_instrument_apply (csrc/instrument_entry.inc)."""
    slots = n_items*TILE
    chunk = GRID_Y
    if slots > 0:
        fit = ((1 << 24)//(slots + 1)//ROW_GROUP)*ROW_GROUP
        chunk = min(chunk, max(fit, ROW_GROUP))
    return min(chunk, rows)


def coverage(instrument, grid):
    """The names of CASES that the channel set reaches on `grid`."""
    t = tiling(instrument, grid)
    begin, end, valid = t["begin"], t["end"], t["valid"]
    lo, hi = instrument.window()
    reached = set()
    v = np.flatnonzero(valid)
    if np.any(begin[v] == 0):
        reached.add("window starts at column 0")
    if np.any(hi[v] == grid[-1]):
        reached.add("window hi is grid[-1]")
    if np.any(end[v] - begin[v] == 1):
        reached.add("window of 1 column")
    from_base = {int(end[c] - t["tiles"][t["tile"][c]]["base"]) for c in v}
    for width in (511, 512, 513):
        if width in from_base:
            reached.add(f"{width} columns from the tile base")
    if np.any(t["n_items"][v] >= 3):
        reached.add("channel spans >= 3 segments")
    if any(tile["items"] < tile["segments"] for tile in t["tiles"]):
        reached.add("tile with a dropped segment")
    if v.size % TILE == 1:
        reached.add("valid channels 16k + 1")
    if any(not valid[c] and np.any(valid[:c]) and np.any(valid[c + 1:])
           for c in range(len(instrument))):
        reached.add("invalid channel between valid")
    centers = instrument.centers[v]
    if np.unique(centers).size < centers.size:
        reached.add("duplicated centre")
    return reached


def channel_weights(instrument, grid, c):
    """Channel c's weights over its columns: Instrument.response restricted to columns()."""
    x = instrument
    keep = [c]
    response = x._response
    if response is not None and response.ndim == 2:
        response = response[keep]
    one = Instrument(x._shape, x._centers[keep],
                     parameter=None if x._parameter is None else x._parameter[keep],
                     half_width=None if x._half_width is None else x._half_width[keep],
                     offsets=x._offsets, response=response)
    start, end = x.columns(grid)
    return one.response(grid)[0, start[c]:end[c]]


_EXTENDED = np.finfo(np.longdouble).nmant >= 63


def _dot(rows, w):
    """rows [R, K] . w [K], summed in extended precision (math.fsum where long double is not)."""
    if _EXTENDED:
        return (rows.astype(np.longdouble) @ w.astype(np.longdouble))
    return np.array([math.fsum(r*w) for r in rows])


def reference(instrument, grid, rows):
    """The channel means of rows [R, len(grid)] (float64) with sums in extended precision, the
    suite's error bound 1e-12 * sum|w v| / |sum w|, and the weights of each channel
    (None where the channel is not valid): NaN where the channel is not covered or its
    weights do not sum to > 0 (as Instrument.apply)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, grid.size)
    n = len(instrument)
    mean = np.full((rows.shape[0], n), np.nan)
    bound = np.zeros((rows.shape[0], n))
    start, end = instrument.columns(grid)
    covered = instrument.covered(grid)
    weights = []
    for c in range(n):
        w = channel_weights(instrument, grid, c) if covered[c] else None
        weights.append(w)
        if w is None or not w.sum() > 0.:
            continue
        total = _dot(np.ones((1, w.size)), w)[0]
        part = rows[:, start[c]:end[c]]
        mean[:, c] = (_dot(part, w)/total).astype(np.float64)
        bound[:, c] = 1e-12*(np.abs(part) @ np.abs(w))/abs(float(total))
    return mean, bound, weights
