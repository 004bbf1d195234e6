"""The surface of compute_radiance (spectral emissivity, reflected downwelling radiance) beside the
plain call at the configs[3] shape on one GPU: 64-level standard atmosphere, synthetic H2O, CO2 and
O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB "total" block), one nadir path behind a
290 K surface whose emissivity table has 11 knots between 0.7 and 0.99.

Reports
  * each kernel alone on a resident 64-level block of the real "total" absorption (synchronous
    calls; minimum and mean of twenty): the emissivity fill (24 MB written per path) with its
    bandwidth against the in-order HBM figure, the plain radiance sweep, the down pass (a plain
    sweep against the direction) and the kSurface up sweep, with its ratio to the plain sweep;
  * the wall time of compute_radiance(band_edges=1 cm-1 bins) without and with the surface
    (median of three after a warm-up) and their ratio.
With --plain-only it runs on a tree without the keywords (the commit before them), for an
interleaved comparison of the plain sweep and the plain call.

    python scripts/surface_timing.py [--out FILE] [--plain-only] [--sweeps-only]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/surface_timing.py --sweeps-only
"""
import numpy as np

from linear_source_timing import timed
from timing_common import PEAK, SURFACE, median_wall, parser, resident_total, setup, write_report

from pylbl_amd.mt_ckd import resident_grid


def main():
    arguments = parser(__doc__)
    arguments.add_argument("--plain-only", action="store_true")
    arguments.add_argument("--sweeps-only", action="store_true")
    args = arguments.parse_args()
    spec, grid, thickness, temperature, edges, starts, report = setup(args.levels)
    knots = np.linspace(600., 3000., 11)
    table = np.array([[0.99, 0.97, 0.9, 0.7, 0.75, 0.95, 0.98, 0.96, 0.93, 0.97, 0.99]])

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    carry, rad, down, rows = (engine.blocks.take(1, n) for _ in range(4))

    def radiance(**more):
        return lambda: engine.path_radiance(
            beta, grid.size, handle, 1, args.levels, 0, thickness, temperature, carry,
            boundary_temperature=[SURFACE], boundary_emissivity=[0.9], radiance=rad, **more)
    sweeps = {"plain": radiance()}
    if not args.plain_only:
        sweeps["down"] = lambda: engine.path_radiance(
            beta, grid.size, handle, 1, args.levels, 0, thickness, temperature, carry,
            radiance=down, from_last=True)
        sweeps["fill"] = lambda: engine.surface_emissivity(handle, rows, knots, table)
        sweeps["up_surface"] = radiance(emissivity_rows=rows, reflection=down)
        sweeps["up_reflection_only"] = radiance(reflection=down)
    for label, sweep in sweeps.items():
        least, mean = timed(sweep)
        report[f"sweep_{label}_min_ms"] = least
        report[f"sweep_{label}_mean_ms"] = mean
    if not args.plain_only:
        report["fill_bytes"] = int(grid.size*16)       # E written, the grid read
        report["fill_fraction_of_peak"] = \
            report["fill_bytes"]/(1e-3*report["sweep_fill_min_ms"])/PEAK
        report["sweep_up_surface_over_plain"] = \
            report["sweep_up_surface_min_ms"]/report["sweep_plain_min_ms"]
        report["sweep_down_over_plain"] = \
            report["sweep_down_min_ms"]/report["sweep_plain_min_ms"]
    for block in (beta, carry, rad, down, rows):
        engine.blocks.give(block)

    if not args.sweeps_only:
        plain = dict(boundary_temperature=SURFACE, boundary_emissivity=0.9, band_edges=edges)
        report["compute_radiance_bands_plain_ms"] = 1e3*median_wall(
            lambda: spec.compute_radiance(thickness, **plain))
        if not args.plain_only:
            report["compute_radiance_bands_surface_ms"] = 1e3*median_wall(
                lambda: spec.compute_radiance(
                    thickness, boundary_temperature=SURFACE, boundary_emissivity=table[0],
                    emissivity_wavenumber=knots, reflection_path_length=1.66*thickness,
                    band_edges=edges))
            report["compute_radiance_surface_over_plain"] = \
                report["compute_radiance_bands_surface_ms"] / \
                report["compute_radiance_bands_plain_ms"]
    write_report(report, args.out)


if __name__ == "__main__":
    main()
