"""lbl_path_thermal_radiance_observer beside lbl_path_thermal_radiance on one GPU: 64 levels x 2^20
points (scatterer_spectral_timing's set-up: the standard atmosphere and synthetic H2O, CO2 and O3
tables on 1 .. 1025 cm-1 at 1/1024 cm-1; a 0.5 GB "total" block), one path, the radiance on the
grid, no bands, a black surface at 290 K, D = 1.66, a view along mu = 0.6; all-clear and with
solar_flux_timing.cloud's grey cloud in levels 8 .. 11.

Timed, each alone on the flux rows lbl_path_thermal_two_stream left in HBM just before the rounds:
  * the flux entry as the radiance calls queue it (the two flux rows per level, nothing else);
  * the existing view entry, lbl_path_thermal_radiance (thermal_view_kernel);
  * the new entry (thermal_observer_kernel) with n_p = L looking down, n_p = L looking up, and
    n_p = L/2 in both directions.
All calls share one engine and the same blocks and are synchronous: the entry returns when its
kernels are done, and the host clock around it is the time.  They take turns, round by round;
reported: minimum (median, maximum) of ROUNDS rounds after one that does not count, and the ratio
of the minima to the existing view entry's.  --existing-only times the flux entry and the existing
view entry alone: the same lines on a library from before the new entry, for the comparison of
the existing entries across commits (run from a checkout of each in turn in one session).

    python scripts/thermal_radiance_observer_timing.py [--out FILE] [--levels N] [--existing-only]
"""
from pathlib import Path
import time

import numpy as np

import timing_common as common
from scatterer_spectral_timing import ROUNDS, spectroscopy
from solar_flux_timing import cloud

from pylbl_amd.paths import DIFFUSIVITY

MU = 0.6


def main():
    parser = common.parser(__doc__)
    parser.add_argument("--existing-only", action="store_true")
    args = parser.parse_args()
    levels = args.levels
    spec, thickness = spectroscopy(levels)
    grid = spec.grid
    temperature = np.ascontiguousarray(spec.atmosphere.temperature, dtype=np.float64).ravel()
    engine, beta, n = common.resident_total(spec)
    handle = engine.load_grid(grid)
    work = engine.blocks.take(2*levels, n)
    up, down = engine.blocks.take(levels, n), engine.blocks.take(levels, n)
    radiance = engine.blocks.take(1, n)

    zeros = np.zeros(levels)
    scatterers = {"all-clear": (zeros, zeros, zeros), "cloud in 4 levels": cloud(levels)}
    fluxes = dict(up_rows=up, down_rows=down)
    shared = dict(diffusivity=DIFFUSIVITY, emissivity=[1.], from_last=True)
    head = (beta, grid.size, handle, 1, levels, 0)

    lines = ["scripts/thermal_radiance_observer_timing.py on one MI355X: %d levels x %d points, "
             "one path, the radiance on the grid." % (levels, grid.size),
             "Times in ms: minimum (median, maximum) of %d synchronous calls that take turns, "
             "after one round that does not count;" % ROUNDS,
             "ratio: the minimum over that of lbl_path_thermal_radiance.", ""]
    for atmosphere, (tau_c, omega_c, g_c) in scatterers.items():
        table = np.ascontiguousarray(
            np.stack([thickness, tau_c, omega_c*tau_c, g_c, temperature], axis=1))

        def flux(table=table):
            engine.path_thermal_two_stream(*head, table, [common.SURFACE], work, **shared,
                                           **fluxes)

        def view(table=table):
            engine.path_thermal_radiance(*head, table, [MU], [common.SURFACE],
                                         radiance_rows=radiance, **shared, **fluxes)

        def observer(passed, view_up, table=table):
            return lambda: engine.path_thermal_radiance_observer(
                *head, table, [MU], np.array([passed], dtype=np.int32), [common.SURFACE], up,
                down, view_up=view_up, radiance_rows=radiance, **shared)

        calls = {"lbl_path_thermal_two_stream": flux, "lbl_path_thermal_radiance": view}
        if not args.existing_only:
            calls.update({"observer, n_p = L, down": observer(levels, False),
                          "observer, n_p = L, up": observer(levels, True),
                          "observer, n_p = L/2, down": observer(levels//2, False),
                          "observer, n_p = L/2, up": observer(levels//2, True)})
        # The flux rows of this atmosphere are in HBM before a view sweep is timed; the flux
        # entry rewrites the same values every round.
        flux()
        times = {label: [] for label in calls}
        for round_ in range(ROUNDS + 1):
            for label, call in calls.items():
                start = time.perf_counter()
                call()
                if round_ > 0:
                    times[label].append((time.perf_counter() - start)*1e3)
        lines.append(atmosphere)
        base = min(times["lbl_path_thermal_radiance"])
        for label, values in times.items():
            lines.append("  %-30s%8.3f (%.3f, %.3f)   ratio %.3f" % (
                label, min(values), float(np.median(values)), max(values), min(values)/base))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    engine.free_grid(handle)
    for block in (beta, work, up, down, radiance):
        engine.blocks.give(block)


if __name__ == "__main__":
    main()
