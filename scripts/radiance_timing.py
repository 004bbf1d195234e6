"""Spectroscopy.compute_radiance at the configs[3] shape on one GPU: 64-level standard
atmosphere, synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB
"total" block).

Reports
  * the radiance sweep alone (Engine.path_radiance on a resident 64-level block of the real
    "total" absorption, synchronous, best of ten) -- radiance, radiance + brightness temperature,
    1 cm-1 band means -- beside the optical-depth sweep (Engine.path_compute) on the same block,
    and the bytes read as a fraction of 6.3 TB/s;
  * the wall time of compute_radiance(band_edges=1 cm-1 bins) and of compute_path with the same
    bands (median of three after a warm-up);
  * the largest relative difference of the 1 cm-1 band means from numpy on the same block.

    python scripts/radiance_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/radiance_timing.py
"""
import numpy as np

from timing_common import PEAK, SURFACE, best_of, median_wall, parser, resident_total, setup, \
    write_report

from pylbl_amd.mt_ckd import resident_grid
from pylbl_amd.spectroscopy import PLANCK_C1, PLANCK_C2


def main():
    args = parser(__doc__).parse_args()
    spec, grid, lengths, temperature, edges, starts, report = setup(args.levels)
    surface = SURFACE

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    carry = engine.blocks.take(1, n)
    rad = engine.blocks.take(1, n)
    bt = engine.blocks.take(1, n)
    band_rad = engine.blocks.take(1, edges.size - 1)
    sweeps = {
        "tau": lambda: engine.path_compute(beta, grid.size, 1, args.levels, 0, lengths, carry,
                                           optical_depth=rad),
        "radiance": lambda: engine.path_radiance(
            beta, grid.size, handle, 1, args.levels, 0, lengths, temperature, carry,
            boundary_temperature=[surface], radiance=rad),
        "radiance+bt": lambda: engine.path_radiance(
            beta, grid.size, handle, 1, args.levels, 0, lengths, temperature, carry,
            boundary_temperature=[surface], radiance=rad, brightness_temperature=bt),
        "radiance_bands": lambda: engine.path_radiance(
            beta, grid.size, handle, 1, args.levels, 0, lengths, temperature, carry,
            boundary_temperature=[surface], radiance=band_rad, band_start=starts),
    }
    read = args.levels*grid.size*8
    report["sweep_bytes_read"] = read
    for label, sweep in sweeps.items():
        best = best_of(sweep)
        report[f"sweep_{label}_ms"] = best*1e3
        report[f"sweep_{label}_fraction_of_6.3TBps"] = read/best/PEAK

    # The same band means in numpy, from the block on the host.
    sweeps["radiance_bands"]()
    got = band_rad.to_host()[0]
    beta_host = beta.to_host()[:, :grid.size]
    nu = grid
    c1nu3 = ((PLANCK_C1*nu)*nu)*nu
    c2nu = PLANCK_C2*nu
    radiance = c1nu3/np.expm1(c2nu/surface)
    for level in range(args.levels):
        x = lengths[level]*beta_host[level]
        radiance = radiance*np.exp(-x) + (c1nu3/np.expm1(c2nu/temperature[level]))*(-np.expm1(-x))
    means = np.add.reduceat(radiance, starts[:-1])/np.diff(starts)
    report["band_mean_radiance_max_relative_difference"] = float(
        np.max(np.abs(got - means)/np.abs(means)))
    del beta_host
    for block in (beta, carry, rad, bt, band_rad):
        engine.blocks.give(block)

    # End to end with 1 cm-1 bands: compute_radiance beside compute_path.
    report["compute_radiance_bands_ms"] = 1e3*median_wall(lambda: spec.compute_radiance(
        lengths, boundary_temperature=surface, band_edges=edges))
    report["compute_path_bands_ms"] = 1e3*median_wall(lambda: spec.compute_path(
        lengths, band_edges=edges))
    write_report(report, args.out)


if __name__ == "__main__":
    main()
