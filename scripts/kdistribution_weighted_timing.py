"""lbl_band_distribution and lbl_band_distribution_weighted at the configs[3] shape on one GPU
(timing_common.setup: 64 levels, 3 M points, a 1.5 GB "total" block), for kdistribution_timing.py's
two band sets -- 10 cm-1 bands (about 10^4 points each) and 16 wide bands (about 2 10^5 points
each) -- with 16 Gauss g intervals and points.

Three sessions take turns in one process, round by round, the block computed afresh before every
call, and each reports the minimum of ten synchronous calls:
  * plain: lbl_band_distribution of this library, the sort alone and with means and quantiles;
  * parent: the same two calls on another build of the library (--parent-library, a build of
    the parent commit; left out without it), on an engine of its own and the same blocks;
  * weighted: lbl_band_distribution_weighted with Planck weights (row temperatures), the pair
    sort alone (pi only) and with the gather, both interval sums, the means and the quantiles.
Then the wall time of compute_kdistribution without and with weighting="planck" (median of three
after a warm-up).  Traffic model: per pass one read and one write of the block at 6.3 TB/s, 8 bytes
per element for the plain sort and 12 for the pair sort; the gather reads 12 and writes 16.

    python scripts/kdistribution_weighted_timing.py [--out FILE] [--levels N]
                                                    [--parent-library FILE]
"""
from ctypes import CDLL, byref, c_int32, c_void_p
from pathlib import Path
import time

import numpy as np

import timing_common as common
from pylbl_amd import abi
from pylbl_amd.paths import g_intervals, interval_columns, quantile_table, g_quadrature_points

CHUNK = 4096        # kSortChunk of csrc/band_sort.h
ROUNDS = 10


class Parent(object):
    """lbl_band_distribution of another build of the library, on an engine of its own."""
    def __init__(self, path):
        self.lib = CDLL(str(Path(path).resolve()))
        for name in ("lbl_engine_create", "lbl_engine_destroy", "lbl_band_distribution"):
            function = getattr(self.lib, name)
            function.argtypes, function.restype = abi.PROTOTYPES[name], c_int32
        self.handle = c_void_p()
        if self.lib.lbl_engine_create(0, byref(self.handle)) != abi.LBL_OK:
            raise RuntimeError("the parent library made no engine.")

    def band_distribution(self, values, columns, starts, scratch, intervals=None, means=None,
                          index=None, fraction=None, quantiles=None):
        status = self.lib.lbl_band_distribution(
            self.handle, values.pointer, values.shape[1], columns, values.shape[0],
            starts.ctypes.data, starts.size - 1, scratch.pointer,
            None if intervals is None else intervals.ctypes.data,
            0 if intervals is None else intervals.size - 1,
            None if means is None else means.pointer,
            None if index is None else index.ctypes.data,
            None if fraction is None else fraction.ctypes.data,
            0 if index is None else index.shape[1],
            None if quantiles is None else quantiles.pointer, 0)
        if status != abi.LBL_OK:
            raise RuntimeError("lbl_band_distribution of the parent library failed.")

    def close(self):
        self.lib.lbl_engine_destroy(self.handle)


def main():
    parser = common.parser(__doc__)
    parser.add_argument("--parent-library", default=None,
                        help="liblbl_amd.so built from the parent commit")
    args = parser.parse_args()
    setup = common.setup(args.levels)
    spec, grid = setup.spec, setup.grid
    levels = args.levels
    engine, beta, n = common.resident_total(spec)
    pairs = (n + 1)//2
    scratch, weight, weighted = (engine.blocks.take(levels, n) for _ in range(3))
    index_rows, index_scratch = (engine.blocks.take(levels, pairs) for _ in range(2))
    handle = engine.load_grid(grid)
    parent = Parent(args.parent_library) if args.parent_library else None
    g = g_intervals(16)
    points = g_quadrature_points(None, 16)
    band_sets = {"10 cm-1 bands": np.arange(1., 3000.5, 10.),
                 "16 wide bands": np.linspace(1., 3000., 17)}
    block_bytes = levels*grid.size*8
    lines = []

    def fresh():
        with engine.pipeline:
            spec.total_into(beta, 0, levels, True)
            engine.synchronize()

    def timed(call):
        fresh()
        start = time.perf_counter()
        call()
        return (time.perf_counter() - start)*1e3

    report = {}
    for name, edges in band_sets.items():
        starts = np.searchsorted(grid, edges).astype(np.int64)
        counts = np.diff(starts)
        intervals = interval_columns(starts, g).ravel()
        index, fraction = quantile_table(counts, points)
        means, sums, more = (engine.blocks.take(levels, intervals.size - 1) for _ in range(3))
        quantiles = engine.blocks.take(levels, index.size)
        merges = max(int(np.ceil(np.log2(max(-(-int(c)//CHUNK), 1)))) for c in counts)
        tables = dict(interval_start=intervals, means=means, point_index=index,
                      point_fraction=fraction, quantiles=quantiles)
        weights = dict(index_scratch=index_scratch, scratch=scratch, grid=handle,
                       row_temperature=setup.temperature)
        calls = {
            "plain, sort alone": lambda: engine.band_distribution(
                beta, grid.size, starts, scratch=scratch),
            "plain, sort + means + quantiles": lambda: engine.band_distribution(
                beta, grid.size, starts, scratch=scratch, **tables),
            "weighted, pair sort alone": lambda: engine.band_distribution_weighted(
                beta, grid.size, starts, index_rows, **weights),
            "weighted, everything": lambda: engine.band_distribution_weighted(
                beta, grid.size, starts, index_rows, weight_rows=weight, weighted_rows=weighted,
                weight_sums=sums, weighted_sums=more, **weights, **tables),
        }
        if parent is not None:
            calls["parent, sort alone"] = lambda: parent.band_distribution(
                beta, grid.size, starts, scratch)
            calls["parent, sort + means + quantiles"] = lambda: parent.band_distribution(
                beta, grid.size, starts, scratch, intervals, means, index, fraction, quantiles)
        times = {label: [] for label in calls}
        for label, call in calls.items():
            timed(call)                                     # (does not count)
        for _ in range(ROUNDS):
            for label, call in calls.items():
                times[label].append(timed(call))
        entry = {"bands": int(counts.size), "points_per_band": int(np.median(counts)),
                 "passes": 1 + merges,
                 "plain_model_ms": (1 + merges)*2*block_bytes/common.PEAK*1e3,
                 "pair_model_ms": ((1 + merges)*3*block_bytes + 3.5*block_bytes)/common.PEAK*1e3}
        for label, values in times.items():
            entry[label] = {"min_ms": min(values), "median_ms": float(np.median(values)),
                            "max_ms": max(values)}
        for blocks in (means, sums, more, quantiles):
            engine.blocks.give(blocks)
        entry["compute_kdistribution_ms"] = common.median_wall(
            lambda: spec.compute_kdistribution(edges, quantities=(
                "absorption_g_mean", "absorption_g_quantile")))*1e3
        entry["compute_kdistribution_planck_ms"] = common.median_wall(
            lambda: spec.compute_kdistribution(edges, quantities=(
                "absorption_g_mean", "absorption_g_quantile", "weight_g_fraction",
                "absorption_g_weighted_mean"), weighting="planck"))*1e3
        report[name] = entry

    names = list(report)
    lines.append("scripts/kdistribution_weighted_timing.py on one MI355X: %d levels x %d points, 16 "
                 "Gauss g intervals and points." % (levels, grid.size))
    lines.append("Times in ms: minimum (median, maximum) of %d synchronous calls, the sessions "
                 "taking turns, the block computed afresh before each." % ROUNDS)
    lines.append("")
    lines.append("%-44s%-28s%-28s" % ("", names[0], names[1]))
    for key, label in (("bands", "bands"), ("points_per_band", "points per band (median)"),
                       ("passes", "passes (chunk sort + merges)")):
        lines.append("%-44s%-28d%-28d" % (label, report[names[0]][key], report[names[1]][key]))
    for key, label in (("plain_model_ms", "traffic model, plain sort (8 B)"),
                       ("pair_model_ms", "traffic model, pair sort (12 B) + gather")):
        lines.append("%-44s%-28.2f%-28.2f" % (label, report[names[0]][key], report[names[1]][key]))
    for label in [x for x in report[names[0]] if isinstance(report[names[0]][x], dict)]:
        cells = ["%.2f (%.2f, %.2f)" % (report[x][label]["min_ms"], report[x][label]["median_ms"],
                                         report[x][label]["max_ms"]) for x in names]
        lines.append("%-44s%-28s%-28s" % (label, cells[0], cells[1]))
    ratio = [report[x]["weighted, pair sort alone"]["min_ms"]/report[x]["plain, sort alone"]["min_ms"]
             for x in names]
    lines.append("%-44s%-28.2f%-28.2f" % ("pair sort alone / plain sort alone", ratio[0], ratio[1]))
    for key, label in (("compute_kdistribution_ms", "compute_kdistribution, end to end"),
                       ("compute_kdistribution_planck_ms", "  with weighting=\"planck\"")):
        lines.append("%-44s%-28.1f%-28.1f" % (label, report[names[0]][key], report[names[1]][key]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    if parent is not None:
        parent.close()
    engine.free_grid(handle)
    for block in (scratch, weight, weighted, index_rows, index_scratch, beta):
        engine.blocks.give(block)


if __name__ == "__main__":
    main()
