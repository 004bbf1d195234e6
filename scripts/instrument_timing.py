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

from pylbl_amd import Instrument, MemoryDatabase, Spectroscopy, synthetic  # noqa: E402
from pylbl_amd import spectroscopy  # noqa: E402
from pylbl_amd.instrument import resident_instrument  # noqa: E402

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
    surface = 290.
    edges = np.arange(1., 3000.5, 1.)
    instrument = Instrument.gaussian(645. + 0.25*np.arange(8461), 0.5, half_width=1.5)
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
    handle = resident_instrument(engine, instrument, spec.grid)
    out = engine.blocks.take(args.levels, len(instrument))
    start, end = instrument.columns(grid)
    covered = int(np.max(end) - np.min(start))
    read = args.levels*covered*8
    report["channels"] = len(instrument)
    report["apply_bytes_read"] = read
    times = []
    for _ in range(11):
        begin = time.perf_counter()
        engine.instrument_apply(beta, args.levels, handle, out)
        times.append(time.perf_counter() - begin)
    best = min(times[1:])
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

    for label, call in (("compute_radiance_instrument_ms", lambda: spec.compute_radiance(
                             lengths, boundary_temperature=surface, instrument=instrument)),
                        ("compute_radiance_bands_ms", lambda: spec.compute_radiance(
                             lengths, boundary_temperature=surface, band_edges=edges))):
        call()
        walls = []
        for _ in range(3):
            begin = time.perf_counter()
            call()
            walls.append(time.perf_counter() - begin)
        report[label] = float(np.median(walls))*1e3
    report["instrument_over_bands"] = report["compute_radiance_instrument_ms"] / \
        report["compute_radiance_bands_ms"]
    print(json.dumps(report, indent=1))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
