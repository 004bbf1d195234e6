"""The linear-in-tau source beside the isothermal one at the configs[3] shape on one GPU: 64-level
standard atmosphere, synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a
1.5 GB "total" block), 3 Gauss-Legendre angles, 290 K black surface; interface temperatures are
the means of neighbouring levels, the outermost those of the end levels.

Reports
  * each sweep alone (Engine.path_radiance, Engine.path_flux down and up on a resident 64-level
    block of the real "total" absorption, synchronous; minimum and mean of twenty) with the
    isothermal and with the linear source, and their ratios;
  * the wall time of compute_flux(band_edges=1 cm-1 bins) with either source (median of three
    after a warm-up).
With --isothermal-only it runs on a tree without the keyword (the commit before it), for an
interleaved comparison of the isothermal sweeps.

    python scripts/linear_source_timing.py [--out FILE] [--isothermal-only]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/linear_source_timing.py
"""
import time

import numpy as np

from timing_common import SURFACE, median_wall, parser, resident_total, setup, write_report

from pylbl_amd.mt_ckd import resident_grid
from pylbl_amd.spectroscopy import flux_angles


def interfaces_of(temperature):
    """[L + 1]: the means of neighbouring levels, the end levels' own values outside."""
    inner = 0.5*(temperature[:-1] + temperature[1:])
    return np.concatenate([temperature[:1], inner, temperature[-1:]])


def timed(call, before=None, count=20):
    """(minimum, mean) [ms] of `count` synchronous calls after one that does not count."""
    times = []
    for _ in range(count + 1):
        if before is not None:
            before()
        start = time.perf_counter()
        call()
        times.append(time.perf_counter() - start)
    return 1e3*min(times[1:]), 1e3*float(np.mean(times[1:]))


def main():
    arguments = parser(__doc__)
    arguments.add_argument("--angles", type=int, default=3)
    arguments.add_argument("--isothermal-only", action="store_true")
    arguments.add_argument("--sweeps-only", action="store_true")
    args = arguments.parse_args()
    spec, grid, thickness, temperature, edges, starts, report = setup(args.levels)
    mu, weight = flux_angles(args.angles)
    lengths = thickness[:, None]/mu
    interfaces = interfaces_of(temperature)
    table = np.ascontiguousarray(np.stack([interfaces[:-1], interfaces[1:]], axis=-1))
    report["angles"] = args.angles
    sources = {"isothermal": {}}
    if not args.isothermal_only:
        sources["linear"] = {"edge_temperature": table}

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    carry = engine.blocks.take(mu.size, n)
    reflection = engine.blocks.take(1, n)
    level = engine.blocks.take(args.levels, n)
    rad = engine.blocks.take(1, n)

    def flux(up, extra):
        return lambda: engine.path_flux(
            beta, grid.size, handle, 1, args.levels, 0, lengths, weight, temperature, carry,
            reflection, level, surface_temperature=[SURFACE], surface_emissivity=[1.], up=up,
            from_last=not up, **extra)
    for source, extra in sources.items():
        down = flux(False, extra)
        sweeps = {
            "radiance": (lambda extra=extra: engine.path_radiance(
                beta, grid.size, handle, 1, args.levels, 0, thickness, temperature, rad,
                boundary_temperature=[SURFACE], radiance=rad, **extra), None),
            "flux_down": (down, None),
            "flux_up": (flux(True, extra), down),      # R for the up sweep, outside the timing
        }
        for label, (sweep, before) in sweeps.items():
            least, mean = timed(sweep, before)
            report[f"sweep_{label}_{source}_min_ms"] = least
            report[f"sweep_{label}_{source}_mean_ms"] = mean
    if "linear" in sources:
        for label in ("radiance", "flux_down", "flux_up"):
            report[f"sweep_{label}_linear_over_isothermal"] = \
                report[f"sweep_{label}_linear_min_ms"]/report[f"sweep_{label}_isothermal_min_ms"]
    for block in (beta, carry, reflection, level, rad):
        engine.blocks.give(block)

    if not args.sweeps_only:
        report["compute_flux_bands_isothermal_ms"] = 1e3*median_wall(lambda: spec.compute_flux(
            thickness, SURFACE, angles=args.angles, band_edges=edges))
        if "linear" in sources:
            report["compute_flux_bands_linear_ms"] = 1e3*median_wall(lambda: spec.compute_flux(
                thickness, SURFACE, angles=args.angles, band_edges=edges,
                source="linear_in_tau", interface_temperature=interfaces))
            report["compute_flux_linear_over_isothermal"] = \
                report["compute_flux_bands_linear_ms"]/report["compute_flux_bands_isothermal_ms"]
    write_report(report, args.out)


if __name__ == "__main__":
    main()
