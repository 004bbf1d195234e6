"""What the spectral scatterer costs in the two radiance calls: lbl_path_thermal_radiance_spectral
and lbl_path_solar_radiance_spectral beside the grey view entries on one GPU, 64 levels x 2^20
points (scatterer_spectral_timing's set-up: the standard atmosphere and synthetic H2O, CO2 and O3
tables on 1 .. 1025 cm-1 at 1/1024 cm-1; a 0.5 GB "total" block), one path, the radiance on the
grid, no bands.  Two things are timed: the view sweep alone, over flux rows that are in HBM, and
the pair a radiance call queues per run, the flux entry and the view entry behind it.

The spectral entries get a table that is flat in wavenumber, with M = 2, 64 and 1024 knots over
the grid, so they compute what the grey entries compute (the same bits); what differs is the work:
the binary search per lane, six values per level and column from the knot rows, the interpolation
and its limit, the products per element and, per element instead of per level, f, gp and a in the
longwave's cloudy levels and the Henyey-Greenstein factor in the shortwave's.  Two atmospheres:
all-clear (no scatterer in any level: the longwave view keeps its clear line in every level) and
solar_flux_timing.cloud's grey cloud in levels 8 .. 11.  The longwave view looks along mu = 0.6
over a black surface at 290 K, the shortwave one along mu = 0.6 and phi = 180 under mu0 = 0.5 over
an albedo of 0.3 with Rayleigh scattering.

All calls share one engine and the same blocks and are synchronous: the entry returns when its
kernels are done, and the host clock around it is the time.  They take turns, round by round;
reported: minimum (median, maximum) of ROUNDS rounds after one that does not count, and the ratio
of the minima to the grey entry's.  --grey-only times the grey entries alone: the same lines on a
library from before the spectral entries, for the comparison of the grey entries across commits.

    python scripts/scatterer_radiance_timing.py [--out FILE] [--levels N] [--grey-only]
"""
from pathlib import Path
import time

import numpy as np

import timing_common as common
from scatterer_spectral_timing import KNOT_COUNTS, ROUNDS, spectroscopy
from solar_flux_timing import ALBEDO, MU0, cloud

from pylbl_amd.paths import DIFFUSIVITY, K_B, SOLAR_SOLID_ANGLE, SOLAR_TEMPERATURE

MU = 0.6
COS_THETA = -MU*MU0 - np.sqrt((1. - MU)*(1. + MU))*np.sqrt((1. - MU0)*(1. + MU0))   # phi = 180


def main():
    parser = common.parser(__doc__)
    parser.add_argument("--grey-only", action="store_true")
    args = parser.parse_args()
    levels = args.levels
    spec, thickness = spectroscopy(levels)
    grid = spec.grid
    temperature = np.ascontiguousarray(spec.atmosphere.temperature, dtype=np.float64).ravel()
    engine, beta, n = common.resident_total(spec)
    handle = engine.load_grid(grid)
    solar, sigma = engine.blocks.take(1, n), engine.blocks.take(1, n)
    work = engine.blocks.take(2*levels, n)
    up, second, third = (engine.blocks.take(levels, n) for _ in range(3))
    radiance = engine.blocks.take(1, n)
    engine.solar_spectrum(handle, solar, grid.size, temperature=SOLAR_TEMPERATURE,
                          scale=SOLAR_SOLID_ANGLE)
    engine.rayleigh_row(handle, sigma, grid.size)

    zeros = np.zeros(levels)
    air = (np.asarray(spec.atmosphere.pressure, dtype=np.float64).ravel() /
           (K_B*temperature))*thickness
    scatterers = {"all-clear": (zeros, zeros, zeros), "cloud in 4 levels": cloud(levels)}

    def flat(tau_c, omega_c, g_c, m):
        knots = np.linspace(grid[0] + 10., grid[-1] - 10., m)
        optics = np.repeat(np.stack([tau_c, omega_c, g_c], axis=1)[:, None, :], m, axis=1)
        return knots, np.ascontiguousarray(optics)

    def longwave(tau_c, omega_c, g_c, m):
        """(the flux entry's call, the view entry's call)."""
        fluxes = dict(up_rows=up, down_rows=second)
        shared = dict(diffusivity=DIFFUSIVITY, emissivity=[1.], from_last=True)
        head = (beta, grid.size, handle, 1, levels, 0)
        if m is None:
            table = np.ascontiguousarray(
                np.stack([thickness, tau_c, omega_c*tau_c, g_c, temperature], axis=1))
            return (lambda: engine.path_thermal_two_stream(
                        *head, table, [common.SURFACE], work, **shared, **fluxes),
                    lambda: engine.path_thermal_radiance(
                        *head, table, [MU], [common.SURFACE], radiance_rows=radiance, **shared,
                        **fluxes))
        table = np.ascontiguousarray(
            np.stack([thickness, zeros, zeros, zeros, temperature], axis=1))
        knots, optics = flat(tau_c, omega_c, g_c, m)
        return (lambda: engine.path_thermal_two_stream_spectral(
                    *head, table, knots, optics, [common.SURFACE], work, **shared, **fluxes),
                lambda: engine.path_thermal_radiance_spectral(
                    *head, table, knots, optics, [MU], [common.SURFACE], radiance_rows=radiance,
                    **shared, **fluxes))

    def shortwave(tau_c, omega_c, g_c, m):
        fluxes = dict(up_rows=up, direct_rows=second, diffuse_rows=third)
        shared = dict(rayleigh_row=sigma, albedo=[ALBEDO], from_last=True)
        if m is None:
            w_c = omega_c*tau_c
            table = np.ascontiguousarray(np.stack([thickness, air, tau_c, w_c, w_c*g_c], axis=1))
            head = (beta, grid.size, 1, levels, 0, table, [MU0])
            return (lambda: engine.path_two_stream(*head, solar, work, **shared, **fluxes),
                    lambda: engine.path_solar_radiance(
                        *head, [MU], [COS_THETA], solar, radiance_rows=radiance, **shared,
                        **fluxes))
        table = np.ascontiguousarray(np.stack([thickness, air, zeros, zeros, zeros], axis=1))
        knots, optics = flat(tau_c, omega_c, g_c, m)
        head = (beta, grid.size, handle, 1, levels, 0, table, knots, optics, [MU0])
        return (lambda: engine.path_two_stream_spectral(*head, solar, work, **shared, **fluxes),
                lambda: engine.path_solar_radiance_spectral(
                    *head, [MU], [COS_THETA], solar, radiance_rows=radiance, **shared, **fluxes))

    entries = {"longwave (lbl_path_thermal_radiance)": longwave,
               "shortwave (lbl_path_solar_radiance)": shortwave}
    counts = () if args.grey_only else KNOT_COUNTS
    lines = ["scripts/scatterer_radiance_timing.py on one MI355X: %d levels x %d points, one "
             "path, the radiance on the grid." % (levels, grid.size),
             "Times in ms: minimum (median, maximum) of %d synchronous calls that take turns, "
             "after one round that does not count;" % ROUNDS,
             "ratio: the minimum over the grey entry's.  The spectral tables are flat: every call "
             "of a block computes the same radiance.", ""]
    for entry, make in entries.items():
        for atmosphere, (tau_c, omega_c, g_c) in scatterers.items():
            made = {"grey": make(tau_c, omega_c, g_c, None)}
            for m in counts:
                made["spectral, M = %d" % m] = make(tau_c, omega_c, g_c, m)
            # The flux rows of this atmosphere are in HBM before a view sweep is timed alone (the
            # spectral tables are flat: every flux entry leaves the same rows).
            made["grey"][0]()

            def pair(flux, view):
                def both():
                    flux()
                    view()
                return both
            for what, calls in (("the view sweep alone",
                                 {label: view for label, (_, view) in made.items()}),
                                ("the flux entry and the view entry",
                                 {label: pair(*two) for label, two in made.items()})):
                times = {label: [] for label in calls}
                for round_ in range(ROUNDS + 1):
                    for label, call in calls.items():
                        start = time.perf_counter()
                        call()
                        if round_ > 0:
                            times[label].append((time.perf_counter() - start)*1e3)
                lines.append("%s, %s, %s" % (entry, atmosphere, what))
                grey = min(times["grey"])
                for label, values in times.items():
                    lines.append("  %-22s%8.3f (%.3f, %.3f)   ratio %.3f" % (
                        label, min(values), float(np.median(values)), max(values),
                        min(values)/grey))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    engine.free_grid(handle)
    for block in (beta, solar, sigma, work, up, second, third, radiance):
        engine.blocks.give(block)


if __name__ == "__main__":
    main()
