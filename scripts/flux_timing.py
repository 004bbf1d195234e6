"""Spectroscopy.compute_flux at the configs[3] shape on one GPU: 64-level standard atmosphere,
synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB "total"
block), 3 Gauss-Legendre angles, 290 K black surface.

Reports
  * each sweep alone (Engine.path_flux down, then up, on a resident 64-level block of the real
    "total" absorption, synchronous, best of ten), on the grid and with 1 cm-1 band means, beside
    the radiance sweep (Engine.path_radiance) on the same block;
  * the wall time of compute_flux(band_edges=1 cm-1 bins) beside compute_radiance with the same
    bands, and beside the 2K calls of compute_radiance (one per angle and direction, path length
    s/mu_k, cumulative) that give the same fluxes with eps = 1 (median of three after a warm-up);
  * the largest relative difference of the emulation's band fluxes from compute_flux's.

    python scripts/flux_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/flux_timing.py
"""
import time

import numpy as np

from timing_common import SURFACE, median_wall, parser, resident_total, setup, \
    write_report

from pylbl_amd import synthetic
from pylbl_amd.mt_ckd import resident_grid
from pylbl_amd.spectroscopy import flux_angles


def emulate(spec, thickness, surface, edges, angles):
    """compute_flux's band fluxes (surface at level 0, eps = 1) from 2K compute_radiance calls."""
    mu, weight = flux_angles(angles)
    down = up = 0.
    for k in range(mu.size):
        s = thickness/mu[k]
        d = spec.compute_radiance(s, direction="toward_first", cumulative=True,
                                  band_edges=edges)["radiance"]
        u = spec.compute_radiance(s, boundary_temperature=surface, direction="toward_last",
                                  cumulative=True, band_edges=edges)["radiance"]
        down = down + weight[k]*d
        up = up + weight[k]*u
    return np.pi*up, np.pi*down


def main():
    arguments = parser(__doc__)
    arguments.add_argument("--angles", type=int, default=3)
    args = arguments.parse_args()
    spec, grid, thickness, temperature, edges, starts, report = setup(args.levels)
    surface = SURFACE
    mu, weight = flux_angles(args.angles)
    lengths = thickness[:, None]/mu
    report["angles"] = args.angles

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    carry = engine.blocks.take(mu.size, n)
    reflection = engine.blocks.take(1, n)
    level = engine.blocks.take(args.levels, n)
    band_flux = engine.blocks.take(args.levels, edges.size - 1)
    band_surface = engine.blocks.take(1, edges.size - 1)
    rad = engine.blocks.take(1, n)

    def flux(up, bands):
        return lambda: engine.path_flux(
            beta, grid.size, handle, 1, args.levels, 0, lengths, weight, temperature, carry,
            reflection, level, surface_temperature=[surface], surface_emissivity=[1.],
            flux=band_flux if bands else None, surface_flux=band_surface if bands and up else None,
            band_start=starts if bands else None, up=up, from_last=not up)
    down_sweep = flux(False, False)
    sweeps = {
        "radiance": lambda: engine.path_radiance(
            beta, grid.size, handle, 1, args.levels, 0, thickness, temperature, rad,
            boundary_temperature=[surface], radiance=rad),
        "flux_down": down_sweep,
        "flux_up": flux(True, False),
        "flux_down_bands": flux(False, True),
        "flux_up_bands": flux(True, True),
    }
    for label, sweep in sweeps.items():
        times = []
        for _ in range(11):
            if label.startswith("flux_up"):
                down_sweep()                    # R for the up sweep, outside the timing
            start = time.perf_counter()
            sweep()
            times.append(time.perf_counter() - start)
        report[f"sweep_{label}_ms"] = min(times[1:])*1e3
    for block in (beta, carry, reflection, level, band_flux, band_surface, rad):
        engine.blocks.give(block)

    # End to end with 1 cm-1 bands.
    report["compute_flux_bands_ms"] = 1e3*median_wall(lambda: spec.compute_flux(
        thickness, surface, angles=args.angles, band_edges=edges))
    report["compute_radiance_bands_ms"] = 1e3*median_wall(lambda: spec.compute_radiance(
        thickness, boundary_temperature=surface, band_edges=edges))
    report["emulation_2K_compute_radiance_ms"] = 1e3*median_wall(lambda: emulate(
        spec, thickness, surface, edges, args.angles))
    report["compute_flux_over_compute_radiance"] = \
        report["compute_flux_bands_ms"]/report["compute_radiance_bands_ms"]
    report["emulation_over_compute_flux"] = \
        report["emulation_2K_compute_radiance_ms"]/report["compute_flux_bands_ms"]

    out = spec.compute_flux(thickness, surface, angles=args.angles, band_edges=edges)
    up, down = emulate(spec, thickness, surface, edges, args.angles)
    _, _, n_per_v = synthetic.grid_arguments(grid)
    width = np.diff(starts)/float(n_per_v)
    worst = 0.
    for got, levels in ((out["upward_flux"][1:], up), (out["downward_flux"][:-1], down)):
        expect = levels*width
        ok = np.isfinite(expect) & (expect != 0.)
        worst = max(worst, float(np.max(np.abs(got[ok] - expect[ok])/np.abs(expect[ok]))))
    report["emulation_max_relative_difference"] = worst
    write_report(report, args.out)


if __name__ == "__main__":
    main()
