"""What radiance_timing.py, flux_timing.py, instrument_timing.py and jacobian_timing.py share: the
configs[3] set-up (64-level standard atmosphere, synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at
0.001 cm-1), the resident "total" block of all its levels, the timers and the report."""
import argparse
from collections import namedtuple
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
from pylbl_amd.engine import default_engine  # noqa: E402

PEAK = 6.3e12       # bytes/s: in-order HBM sweeps on the MI355X
SURFACE = 290.      # [K]

Setup = namedtuple("Setup", ["spec", "grid", "lengths", "temperature", "edges", "starts",
                             "report"])


def parser(doc):
    """--out and --levels, which every script takes."""
    parser = argparse.ArgumentParser(description=doc.splitlines()[0])
    parser.add_argument("--out", default=None, help="also write the report (JSON) here")
    parser.add_argument("--levels", type=int, default=64)
    return parser


def setup(levels):
    """The Spectroscopy, its grid, a nadir path (the layer thicknesses of the scale-height
    altitudes [m], level 0 at the surface), the level temperatures, 1 cm-1 band edges with their
    column starts, and the report's first entries."""
    gases = ("H2O", "CO2", "O3")
    tables = [synthetic.line_table(name, 1., 3000.) for name in gases]
    full = synthetic.standard_atmosphere(levels)
    atmos = synthetic.Atmos(p=full.p, t=full.t, vmr={k: full.vmr[k] for k in gases})
    grid = np.arange(1., 3000., 0.001)
    spec = Spectroscopy(atmos, grid, MemoryDatabase(tables))
    z = -7000.*np.log(full.p/101325.)
    edges = np.arange(1., 3000.5, 1.)
    report = {"levels": levels, "points": int(grid.size),
              "lines": [int(t.num_lines) for t in tables]}
    return Setup(spec, grid, np.gradient(z), np.ascontiguousarray(full.t, dtype=np.float64),
                 edges, np.searchsorted(grid, edges), report)


def iasi_like():
    """Gaussian, FWHM 0.5 cm-1, half width 1.5 cm-1, centres 645.00 ... 2760.00 every 0.25 cm-1."""
    return Instrument.gaussian(645. + 0.25*np.arange(8461), 0.5, half_width=1.5)


def resident_total(spec):
    """(engine, beta, n): the "total" block of all levels in HBM, queued as the path products
    queue it (pedestal removed), finished; n its row length."""
    engine = default_engine(spec.device)
    v0, vn, n_per_v = synthetic.grid_arguments(spec.grid)
    n = (vn - v0)*n_per_v
    levels = spec.atmosphere.temperature.size
    beta = engine.blocks.take(levels, n)
    with engine.pipeline:
        spec.total_into(beta, 0, levels, True)
        engine.synchronize()
    return engine, beta, n


def best_of(call, count=10):
    """Seconds: the best of `count` calls after one that does not count."""
    times = []
    for _ in range(count + 1):
        start = time.perf_counter()
        call()
        times.append(time.perf_counter() - start)
    return min(times[1:])


def median_wall(call, count=3):
    """Seconds: the median of `count` calls after a warm-up."""
    call()
    walls = []
    for _ in range(count):
        start = time.perf_counter()
        call()
        walls.append(time.perf_counter() - start)
    return float(np.median(walls))


def write_report(report, out=None):
    print(json.dumps(report, indent=1))
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(report, indent=1) + "\n")
