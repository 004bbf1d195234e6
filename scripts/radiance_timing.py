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

PEAK = 6.3e12       # bytes/s: in-order HBM sweeps on the MI355X


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--out", default=None, help="also write the report (JSON) here")
    parser.add_argument("--levels", type=int, default=64)
    args = parser.parse_args()

    gases = ("H2O", "CO2", "O3")
    tables = [synthetic.line_table(name, 1., 3000.) for name in gases]
    full = synthetic.standard_atmosphere(args.levels)
    atmos = synthetic.Atmos(p=full.p, t=full.t, vmr={k: full.vmr[k] for k in gases})
    grid = np.arange(1., 3000., 0.001)
    spec = Spectroscopy(atmos, grid, MemoryDatabase(tables))
    # A nadir path: the layer thicknesses of the scale-height altitudes [m].
    z = -7000.*np.log(full.p/101325.)
    lengths = np.gradient(z)
    temperature = np.ascontiguousarray(full.t, dtype=np.float64)
    surface = 290.
    edges = np.arange(1., 3000.5, 1.)
    starts = np.searchsorted(grid, edges)
    report = {"levels": args.levels, "points": int(grid.size),
              "lines": [int(t.num_lines) for t in tables]}

    # The "total" block of all levels in HBM, queued as compute_radiance queues it.
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
        times = []
        for _ in range(11):
            start = time.perf_counter()
            sweep()
            times.append(time.perf_counter() - start)
        best = min(times[1:])
        report[f"sweep_{label}_ms"] = best*1e3
        report[f"sweep_{label}_fraction_of_6.3TBps"] = read/best/PEAK

    # The same band means in numpy, from the block on the host.
    sweeps["radiance_bands"]()
    got = band_rad.to_host()[0]
    beta_host = beta.to_host()[:, :grid.size]
    nu = grid
    c1nu3 = ((spectroscopy.PLANCK_C1*nu)*nu)*nu
    c2nu = spectroscopy.PLANCK_C2*nu
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
    for label, call in (("compute_radiance_bands_ms", lambda: spec.compute_radiance(
                             lengths, boundary_temperature=surface, band_edges=edges)),
                        ("compute_path_bands_ms", lambda: spec.compute_path(
                             lengths, band_edges=edges))):
        call()
        walls = []
        for _ in range(3):
            start = time.perf_counter()
            call()
            walls.append(time.perf_counter() - start)
        report[label] = float(np.median(walls))*1e3
    print(json.dumps(report, indent=1))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
