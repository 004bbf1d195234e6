"""Instrument line shapes at the configs[3] shape on one GPU: 64-level standard atmosphere,
synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB "total"
block), and an IASI-like Gaussian: FWHM 0.5 cm-1, half width 1.5 cm-1, centres 645.00 ...
2760.00 every 0.25 cm-1 (8461 channels).

Reports
  * the apply step alone (Engine.instrument_apply on the 64 resident rows of the real "total"
    absorption, synchronous, best of ten), and the bytes of the covered columns read as a
    fraction of 6.3 TB/s;
  * the largest relative difference from numpy (Instrument.apply) on 8 of those rows;
  * the wall time of compute_radiance(instrument=...) beside compute_radiance(band_edges=1 cm-1
    bins) (median of three after a warm-up).
The kernel times come from a run under rocprofv3:

    python scripts/instrument_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/instrument_timing.py
"""
import numpy as np

from timing_common import PEAK, SURFACE, best_of, iasi_like, median_wall, parser, \
    resident_total, setup, write_report

from pylbl_amd import Instrument
from pylbl_amd.instrument import resident_instrument


def main():
    args = parser(__doc__).parse_args()
    spec, grid, lengths, _, edges, _, report = setup(args.levels)
    surface = SURFACE
    instrument = iasi_like()

    engine, beta, n = resident_total(spec)
    handle = resident_instrument(engine, instrument, spec.grid)
    out = engine.blocks.take(args.levels, len(instrument))
    start, end = instrument.columns(grid)
    covered = int(np.max(end) - np.min(start))
    read = args.levels*covered*8
    report["channels"] = len(instrument)
    report["apply_bytes_read"] = read
    best = best_of(lambda: engine.instrument_apply(beta, args.levels, handle, out))
    report["apply_ms"] = best*1e3
    report["apply_fraction_of_6.3TBps"] = read/best/PEAK

    # numpy on every 40th channel, over its window only (the dense [8461, 3 M] response would
    # not fit in host memory).
    got = out.to_host()[:8]
    rows = beta.to_host()[:8, :grid.size]
    worst = 0.
    for c in range(0, len(instrument), 40):
        one = Instrument.gaussian(instrument.centers[c:c + 1], 0.5, half_width=1.5)
        window = slice(int(start[c]), int(end[c]))
        w = one.response(grid[window])[0]
        expected = (rows[:, window] @ w)/np.sum(w)
        worst = max(worst, float(np.max(np.abs(got[:, c] - expected)/np.abs(expected))))
    report["apply_max_relative_difference_every_40th_channel"] = worst
    del rows
    for block in (beta, out):
        engine.blocks.give(block)

    report["compute_radiance_instrument_ms"] = 1e3*median_wall(lambda: spec.compute_radiance(
        lengths, boundary_temperature=surface, instrument=instrument))
    report["compute_radiance_bands_ms"] = 1e3*median_wall(lambda: spec.compute_radiance(
        lengths, boundary_temperature=surface, band_edges=edges))
    report["instrument_over_bands"] = report["compute_radiance_instrument_ms"] / \
        report["compute_radiance_bands_ms"]
    write_report(report, args.out)


if __name__ == "__main__":
    main()
