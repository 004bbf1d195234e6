"""Spectroscopy.compute_solar at the configs[3] shape on one GPU: 64-level standard atmosphere,
synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB "total"
block), the Sun at mu0 = 0.5 over a surface of albedo 0.3 seen from space at nadir.

Reports, interleaved in one session (minimum and mean of ten after one call that does not count)
  * each sweep alone on a resident 64-level block of the real "total" absorption, synchronous,
    with 1 cm-1 band means: Engine.path_compute with cumulative transmittance (the baseline),
    Engine.path_solar without and with a viewer, and the fill of the S row;
  * the wall time of compute_solar(band_edges=1 cm-1 bins), direct beam alone and with the
    reflected radiance, beside compute_path(cumulative=, band_edges=) on the same paths.

    python scripts/solar_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/solar_timing.py
"""
import time

import numpy as np

from timing_common import parser, resident_total, setup, write_report

from pylbl_amd.mt_ckd import resident_grid
from pylbl_amd.paths import SOLAR_SOLID_ANGLE, SOLAR_TEMPERATURE

MU0, ALBEDO = 0.5, 0.3


def interleaved(calls, count=10):
    """{label: (min, mean) [ms]} of `count` rounds over all the calls, after one round that does
    not count."""
    times = {label: [] for label in calls}
    for _ in range(count + 1):
        for label, call in calls.items():
            start = time.perf_counter()
            call()
            times[label].append(time.perf_counter() - start)
    return {label: (1e3*min(t[1:]), 1e3*float(np.mean(t[1:]))) for label, t in times.items()}


def main():
    args = parser(__doc__).parse_args()
    spec, grid, thickness, temperature, edges, starts, report = setup(args.levels)
    slant = thickness/MU0
    bands = edges.size - 1

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    carry = engine.blocks.take(2, n)
    solar = engine.blocks.take(1, n)
    level = engine.blocks.take(args.levels, n)
    space, reflected = engine.blocks.take(1, n), engine.blocks.take(1, n)
    level_mean = engine.blocks.take(args.levels, bands)
    space_mean, reflected_mean = engine.blocks.take(1, bands), engine.blocks.take(1, bands)
    path_carry = carry.rows(1)

    def fill():
        engine.solar_spectrum(handle, solar, grid.size, temperature=SOLAR_TEMPERATURE,
                              scale=SOLAR_SOLID_ANGLE)
    fill()

    def sweep(view):
        more = dict(view_lengths=thickness, albedo=[ALBEDO], reflected_rows=reflected,
                    reflected_mean=reflected_mean) if view else {}
        return lambda: engine.path_solar(
            beta, grid.size, 1, args.levels, 0, slant, [MU0], solar, carry, interface_rows=level,
            space_rows=space, interface_mean=level_mean, space_mean=space_mean,
            band_start=starts, from_last=True, **more)
    baseline = lambda: engine.path_compute(
        beta, grid.size, 1, args.levels, 0, slant, path_carry, transmittance=level_mean,
        band_start=starts, cumulative=True, from_last=True)
    # path_compute with bands and cumulative forms tau in place, over beta: it goes last in every
    # round, and the solar sweeps of the next round read what it left -- the same bytes moved and
    # the same instructions, whatever the values.
    for label, (low, mean) in interleaved({"solar_spectrum": fill, "path_solar": sweep(False),
                                           "path_solar_view": sweep(True),
                                           "path_sweep_transmittance": baseline}).items():
        report[f"sweep_{label}_min_ms"], report[f"sweep_{label}_mean_ms"] = low, mean
    report["path_solar_over_path_sweep"] = \
        report["sweep_path_solar_min_ms"]/report["sweep_path_sweep_transmittance_min_ms"]
    report["path_solar_view_over_path_sweep"] = \
        report["sweep_path_solar_view_min_ms"]/report["sweep_path_sweep_transmittance_min_ms"]
    for block in (beta, carry, solar, level, space, reflected, level_mean, space_mean,
                  reflected_mean):
        engine.blocks.give(block)

    # End to end with 1 cm-1 bands.
    calls = {
        "compute_path_cumulative": lambda: spec.compute_path(
            slant, quantities="transmittance", cumulative="from_last", band_edges=edges),
        "compute_solar_direct": lambda: spec.compute_solar(thickness, MU0, band_edges=edges),
        "compute_solar_reflected": lambda: spec.compute_solar(
            thickness, MU0, surface_albedo=ALBEDO, view_path_length=thickness, band_edges=edges,
            quantities=("direct_irradiance", "reflected_radiance")),
    }
    for label, (low, mean) in interleaved(calls, count=5).items():
        report[f"{label}_min_ms"], report[f"{label}_mean_ms"] = low, mean
    report["compute_solar_over_compute_path"] = \
        report["compute_solar_direct_min_ms"]/report["compute_path_cumulative_min_ms"]
    write_report(report, args.out)


if __name__ == "__main__":
    main()
