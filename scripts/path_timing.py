"""Spectroscopy.compute_path at the configs[3] shape on one GPU: 64-level standard atmosphere,
synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB "total" block).

Reports
  * the path sweep alone (Engine.path_compute on a resident 64-level block, synchronous, best of
    ten) and the bytes it reads as a fraction of 6.3 TB/s;
  * the wall time of compute_path(band_edges=1 cm-1 bins) (median of three after a warm-up);
  * the wall time of compute_absorption("total") followed by the same reduction in numpy.

    python scripts/path_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/path_timing.py
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
    edges = np.arange(1., 3000.5, 1.)
    report = {"levels": args.levels, "points": int(grid.size),
              "lines": [int(t.num_lines) for t in tables]}

    # The sweep alone on a resident block.
    engine = spec._molecule("H2O").gas.engine
    v0, vn, n_per_v = synthetic.grid_arguments(grid)
    n = (vn - v0)*n_per_v
    beta = engine.blocks.take(args.levels, n)
    carry = engine.blocks.take(1, n)
    tau = engine.blocks.take(1, n)
    trans = engine.blocks.take(1, n)
    engine.fill_zero(beta)
    best = {}
    for label, keywords in (("tau", dict(optical_depth=tau)),
                            ("tau+trans", dict(optical_depth=tau, transmittance=trans)),
                            ("bands", dict(optical_depth=tau, transmittance=trans,
                                           band_start=np.searchsorted(grid, edges)))):
        if label == "bands":
            keywords["optical_depth"] = engine.blocks.take(1, edges.size - 1)
            keywords["transmittance"] = engine.blocks.take(1, edges.size - 1)
        times = []
        for _ in range(11):
            start = time.perf_counter()
            engine.path_compute(beta, grid.size, 1, args.levels, 0, lengths, carry, **keywords)
            times.append(time.perf_counter() - start)
        best[label] = min(times[1:])
    read = args.levels*grid.size*8
    report["sweep_bytes_read"] = read
    for label, seconds in best.items():
        report[f"sweep_{label}_ms"] = seconds*1e3
        report[f"sweep_{label}_fraction_of_6.3TBps"] = read/seconds/PEAK
    for block in (beta, carry, tau, trans):
        engine.blocks.give(block)

    # compute_path with 1 cm-1 bands, end to end.
    spec.compute_path(lengths, band_edges=edges)
    walls = []
    for _ in range(3):
        start = time.perf_counter()
        out = spec.compute_path(lengths, band_edges=edges)
        walls.append(time.perf_counter() - start)
    report["compute_path_bands_ms"] = float(np.median(walls))*1e3

    # The same through the host: the block comes home, numpy integrates and averages.
    spec.compute_absorption("total")
    start = time.perf_counter()
    beta_host = np.asarray(spec.compute_absorption("total")["absorption"])
    middle = time.perf_counter()
    tau_host = np.zeros(grid.size)
    for level in range(args.levels):
        tau_host = tau_host + lengths[level]*beta_host[level]
    starts = np.searchsorted(grid, edges)
    trans_host = np.exp(-tau_host)
    means = np.add.reduceat(trans_host, starts[:-1])/np.diff(starts)
    end = time.perf_counter()
    report["compute_absorption_total_ms"] = (middle - start)*1e3
    report["numpy_reduction_ms"] = (end - middle)*1e3
    report["host_route_ms"] = (end - start)*1e3
    # (bands where the transmittance underflows to 0 compare absolutely)
    error = np.max(np.abs(out["transmittance"] - means)/np.maximum(np.abs(means), 1.e-300))
    report["band_mean_transmittance_max_relative_difference"] = float(error)
    print(json.dumps(report, indent=1))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
