"""Spectroscopy.compute_kdistribution at the configs[3] shape on one GPU (timing_common.setup: 64
levels, 3 M points, a 1.5 GB "total" block), for 10 cm-1 bands (about 10^4 points each) and for 16
wide bands (about 2 10^5 points each), 16 Gauss g intervals.

Reports, per band set,
  * lbl_band_distribution alone on the resident block (Engine.band_distribution, synchronous, the
    block computed afresh before each of three calls, the best of them): the sort alone, and the
    sort with the interval means and the quantiles; the sort's passes (1 chunk sort + merge
    passes) and its traffic model -- one read and one write of the block per pass at 6.3 TB/s;
  * the wall time of compute_kdistribution (median of three after a warm-up);
  * the host route: compute_absorption("total"), then numpy.sort and the interval means per band
    and level on one core.

    python scripts/kdistribution_timing.py [--out FILE] [--levels N]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/kdistribution_timing.py
"""
import time

import numpy as np

import timing_common as common
from pylbl_amd.paths import g_intervals, interval_columns, quantile_table, g_quadrature_points

CHUNK = 4096        # kSortChunk of csrc/band_sort.h


def main():
    args = common.parser(__doc__).parse_args()
    setup = common.setup(args.levels)
    spec, grid, report = setup.spec, setup.grid, setup.report
    levels = args.levels
    engine, beta, n = common.resident_total(spec)
    scratch = engine.blocks.take(levels, n)
    g = g_intervals(16)
    points = g_quadrature_points(None, 16)
    band_sets = {"10cm-1": np.arange(1., 3000.5, 10.),
                 "16 wide": np.linspace(1., 3000., 17)}
    block_bytes = levels*grid.size*8

    def fresh():
        with engine.pipeline:
            spec.total_into(beta, 0, levels, True)
            engine.synchronize()

    for name, edges in band_sets.items():
        starts = np.searchsorted(grid, edges).astype(np.int64)
        counts = np.diff(starts)
        intervals = interval_columns(starts, g).ravel()
        index, fraction = quantile_table(counts, points)
        means = engine.blocks.take(levels, intervals.size - 1)
        quantiles = engine.blocks.take(levels, index.size)
        passes = 1 + max(int(np.ceil(np.log2(max(-(-int(c)//CHUNK), 1)))) for c in counts)
        entry = {"bands": int(counts.size), "points_per_band": int(np.median(counts)),
                 "passes": passes, "model_ms": passes*2*block_bytes/common.PEAK*1e3}
        for label, keywords in (
                ("sort", {}),
                ("sort+means+quantiles", dict(interval_start=intervals, means=means,
                                              point_index=index, point_fraction=fraction,
                                              quantiles=quantiles))):
            times = []
            for _ in range(3):
                fresh()
                start = time.perf_counter()
                engine.band_distribution(beta, grid.size, starts, scratch=scratch, **keywords)
                times.append(time.perf_counter() - start)
            entry[label + "_ms"] = min(times)*1e3
        entry["sort_fraction_of_model"] = entry["model_ms"]/entry["sort_ms"]
        engine.blocks.give(means)
        engine.blocks.give(quantiles)

        entry["compute_kdistribution_ms"] = common.median_wall(
            lambda: spec.compute_kdistribution(edges, quantities=(
                "absorption_g_mean", "absorption_g_quantile")))*1e3

        # The host route: the block comes home, numpy sorts every band of every level.
        spec.compute_absorption("total")
        start = time.perf_counter()
        host = np.asarray(spec.compute_absorption("total")["absorption"])
        middle = time.perf_counter()
        bounds = interval_columns(starts, g)
        out = np.full((levels, counts.size, g.size - 1), np.nan)
        for level in range(levels):
            for b in range(counts.size):
                band = np.sort(host[level, starts[b]:starts[b + 1]])
                cuts = bounds[b] - starts[b]
                for q in range(g.size - 1):
                    if cuts[q + 1] > cuts[q]:
                        out[level, b, q] = band[cuts[q]:cuts[q + 1]].mean()
        end = time.perf_counter()
        entry["compute_absorption_total_ms"] = (middle - start)*1e3
        entry["numpy_sort_and_means_ms"] = (end - middle)*1e3
        entry["host_route_ms"] = (end - start)*1e3
        report[name] = entry
    engine.blocks.give(scratch)
    engine.blocks.give(beta)
    common.write_report(report, args.out)


if __name__ == "__main__":
    main()
