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
import argparse
import json
import os
from pathlib import Path
import sys
import time

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("PYLBL_MT_CKD", str(ROOT / "tests" / "golden" / "mt_ckd_bands.npz"))

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic  # noqa: E402
from pylbl_amd import spectroscopy  # noqa: E402
from pylbl_amd.mt_ckd import resident_grid  # noqa: E402


def wall(call):
    call()
    walls = []
    for _ in range(3):
        start = time.perf_counter()
        call()
        walls.append(time.perf_counter() - start)
    return float(np.median(walls))*1e3


def emulate(spec, thickness, surface, edges, angles):
    """compute_flux's band fluxes (surface at level 0, eps = 1) from 2K compute_radiance calls."""
    mu, weight = spectroscopy.flux_angles(angles)
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
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--out", default=None, help="also write the report (JSON) here")
    parser.add_argument("--levels", type=int, default=64)
    parser.add_argument("--angles", type=int, default=3)
    args = parser.parse_args()

    gases = ("H2O", "CO2", "O3")
    tables = [synthetic.line_table(name, 1., 3000.) for name in gases]
    full = synthetic.standard_atmosphere(args.levels)
    atmos = synthetic.Atmos(p=full.p, t=full.t, vmr={k: full.vmr[k] for k in gases})
    grid = np.arange(1., 3000., 0.001)
    spec = Spectroscopy(atmos, grid, MemoryDatabase(tables))
    # The layer thicknesses of the scale-height altitudes [m]; level 0 at the surface.
    z = -7000.*np.log(full.p/101325.)
    thickness = np.gradient(z)
    temperature = np.ascontiguousarray(full.t, dtype=np.float64)
    surface = 290.
    edges = np.arange(1., 3000.5, 1.)
    starts = np.searchsorted(grid, edges)
    mu, weight = spectroscopy.flux_angles(args.angles)
    lengths = thickness[:, None]/mu
    report = {"levels": args.levels, "points": int(grid.size), "angles": args.angles,
              "lines": [int(t.num_lines) for t in tables]}

    # The "total" block of all levels in HBM, queued as compute_flux queues it.
    temperature_flat = spec.atmosphere.temperature.ravel()
    pressure = spec.atmosphere.pressure.ravel()
    fractions = {k: v.ravel() for k, v in spec.atmosphere.gases.items()}
    engine, present, heavy = spec._present_gases(temperature_flat, pressure, fractions)
    if heavy is not None:
        present = [heavy] + present[:-1]
    v0, vn, n_per_v = synthetic.grid_arguments(grid)
    n = (vn - v0)*n_per_v
    beta = engine.blocks.take(args.levels, n)
    with engine.pipeline:
        queue = spectroscopy._Queue(spec, temperature_flat, pressure, fractions, True,
                                    "reference", spec.delivery_pieces)
        spec._queue_total(queue, engine, present, heavy,
                          spectroscopy._Sum(engine, args.levels, n, buffer=beta), None)
        engine.synchronize()
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
    sweeps = {
        "radiance": lambda: engine.path_radiance(
            beta, grid.size, handle, 1, args.levels, 0, thickness, temperature, rad,
            boundary_temperature=[surface], radiance=rad),
        "flux_down": flux(False, False),
        "flux_up": flux(True, False),
        "flux_down_bands": flux(False, True),
        "flux_up_bands": flux(True, True),
    }
    for label, sweep in sweeps.items():
        times = []
        for _ in range(11):
            if label.startswith("flux_up"):
                flux(False, False)()            # R for the up sweep, outside the timing
            start = time.perf_counter()
            sweep()
            times.append(time.perf_counter() - start)
        report[f"sweep_{label}_ms"] = min(times[1:])*1e3
    for block in (beta, carry, reflection, level, band_flux, band_surface, rad):
        engine.blocks.give(block)

    # End to end with 1 cm-1 bands.
    report["compute_flux_bands_ms"] = wall(lambda: spec.compute_flux(
        thickness, surface, angles=args.angles, band_edges=edges))
    report["compute_radiance_bands_ms"] = wall(lambda: spec.compute_radiance(
        thickness, boundary_temperature=surface, band_edges=edges))
    report["emulation_2K_compute_radiance_ms"] = wall(lambda: emulate(
        spec, thickness, surface, edges, args.angles))
    report["compute_flux_over_compute_radiance"] = \
        report["compute_flux_bands_ms"]/report["compute_radiance_bands_ms"]
    report["emulation_over_compute_flux"] = \
        report["emulation_2K_compute_radiance_ms"]/report["compute_flux_bands_ms"]

    out = spec.compute_flux(thickness, surface, angles=args.angles, band_edges=edges)
    up, down = emulate(spec, thickness, surface, edges, args.angles)
    width = np.diff(starts)/float(n_per_v)
    worst = 0.
    for got, levels in ((out["upward_flux"][1:], up), (out["downward_flux"][:-1], down)):
        expect = levels*width
        ok = np.isfinite(expect) & (expect != 0.)
        worst = max(worst, float(np.max(np.abs(got[ok] - expect[ok])/np.abs(expect[ok]))))
    report["emulation_max_relative_difference"] = worst
    print(json.dumps(report, indent=1))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
