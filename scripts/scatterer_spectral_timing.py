"""What the spectral scatterer costs: lbl_path_two_stream_spectral and
lbl_path_thermal_two_stream_spectral beside the grey entries on one GPU, 64 levels x 2^20 points
(the standard atmosphere and synthetic H2O, CO2 and O3 tables of the other timing scripts on
1 .. 1025 cm-1 at 1/1024 cm-1; a 0.5 GB "total" block), one path, upward and downward fluxes on the
grid, no bands.

The spectral entries get a table that is flat in wavenumber, with M = 2, 64 and 1024 knots over
the grid, so they compute what the grey entry computes (the same bits); what differs is the work:
the binary search per lane, six values per level and column from the knot rows, the interpolation
and its limit, the products per element and, in the longwave's cloudy levels, f and gp per
element.  Two atmospheres: all-clear (no scatterer in any level: the longwave entries keep their
clear branch in every level) and solar_flux_timing.cloud's grey cloud in levels 8 .. 11.  Three
entries: the shortwave one (mu0 = 0.5, albedo 0.3, Rayleigh scattering) and the longwave one with
the level-temperature source and with the linear-in-tau source.

All calls share one engine and the same blocks and are synchronous: the entry returns when its
kernels are done, and the host clock around it is the time.  They take turns, round by round;
reported: minimum (median, maximum) of ROUNDS rounds after one that does not count, and the ratio
of the minima to the grey entry's.

    python scripts/scatterer_spectral_timing.py [--out FILE] [--levels N]
"""
from pathlib import Path
import time

import numpy as np

import timing_common as common
from solar_flux_timing import ALBEDO, MU0, cloud

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd.paths import DIFFUSIVITY, K_B, SOLAR_SOLID_ANGLE, SOLAR_TEMPERATURE

ROUNDS = 20
KNOT_COUNTS = (2, 64, 1024)
POINTS_PER_WAVENUMBER = 1024        # 1 .. 1025 cm-1: 2^20 points


def spectroscopy(levels):
    """timing_common.setup's atmosphere and gases on 2^20 points: (spec, thickness [m])."""
    gases = ("H2O", "CO2", "O3")
    tables = [synthetic.line_table(name, 1., 1025.) for name in gases]
    full = synthetic.standard_atmosphere(levels)
    atmos = synthetic.Atmos(p=full.p, t=full.t, vmr={k: full.vmr[k] for k in gases})
    grid = 1. + np.arange(1024*POINTS_PER_WAVENUMBER)/float(POINTS_PER_WAVENUMBER)
    spec = Spectroscopy(atmos, grid, MemoryDatabase(tables))
    return spec, np.gradient(-7000.*np.log(full.p/101325.))


def main():
    args = common.parser(__doc__).parse_args()
    levels = args.levels
    spec, thickness = spectroscopy(levels)
    grid = spec.grid
    temperature = np.ascontiguousarray(spec.atmosphere.temperature, dtype=np.float64).ravel()
    engine, beta, n = common.resident_total(spec)
    handle = engine.load_grid(grid)
    solar, sigma = engine.blocks.take(1, n), engine.blocks.take(1, n)
    work = engine.blocks.take(2*levels, n)
    up, down = engine.blocks.take(levels, n), engine.blocks.take(levels, n)
    top_up, top_down = engine.blocks.take(1, n), engine.blocks.take(1, n)
    engine.solar_spectrum(handle, solar, grid.size, temperature=SOLAR_TEMPERATURE,
                          scale=SOLAR_SOLID_ANGLE)
    engine.rayleigh_row(handle, sigma, grid.size)
    outputs = dict(up_rows=up, down_rows=down, top_up_rows=top_up, top_down_rows=top_down,
                   from_last=True)

    zeros = np.zeros(levels)
    air = (np.asarray(spec.atmosphere.pressure, dtype=np.float64).ravel() /
           (K_B*temperature))*thickness
    interfaces = np.concatenate([temperature[:1], (temperature[:-1] + temperature[1:])/2.,
                                 temperature[-1:]])
    edges = np.ascontiguousarray(np.stack([interfaces[:-1], interfaces[1:]], axis=1))
    scatterers = {"all-clear": (zeros, zeros, zeros), "cloud in 4 levels": cloud(levels)}

    def shortwave(tau_c, omega_c, g_c, m):
        w_c = omega_c*tau_c
        if m is None:
            table = np.ascontiguousarray(np.stack([thickness, air, tau_c, w_c, w_c*g_c], axis=1))
            return lambda: engine.path_two_stream(
                beta, grid.size, 1, levels, 0, table, [MU0], solar, work, rayleigh_row=sigma,
                albedo=[ALBEDO], **outputs)
        table = np.ascontiguousarray(np.stack([thickness, air, zeros, zeros, zeros], axis=1))
        knots, optics = flat(tau_c, omega_c, g_c, m)
        return lambda: engine.path_two_stream_spectral(
            beta, grid.size, handle, 1, levels, 0, table, knots, optics, [MU0], solar, work,
            rayleigh_row=sigma, albedo=[ALBEDO], **outputs)

    def longwave(linear):
        def make(tau_c, omega_c, g_c, m):
            common_ = dict(diffusivity=DIFFUSIVITY, emissivity=[1.], **outputs)
            if m is None:
                table = np.ascontiguousarray(
                    np.stack([thickness, tau_c, omega_c*tau_c, g_c, temperature], axis=1))
                if linear:
                    return lambda: engine.path_thermal_two_stream_source(
                        beta, grid.size, handle, 1, levels, 0, table, edges, [common.SURFACE],
                        work, **common_)
                return lambda: engine.path_thermal_two_stream(
                    beta, grid.size, handle, 1, levels, 0, table, [common.SURFACE], work,
                    **common_)
            table = np.ascontiguousarray(
                np.stack([thickness, zeros, zeros, zeros, temperature], axis=1))
            knots, optics = flat(tau_c, omega_c, g_c, m)
            return lambda: engine.path_thermal_two_stream_spectral(
                beta, grid.size, handle, 1, levels, 0, table, knots, optics, [common.SURFACE],
                work, edge_temperature=edges if linear else None, **common_)
        return make

    def flat(tau_c, omega_c, g_c, m):
        knots = np.linspace(grid[0] + 10., grid[-1] - 10., m)
        optics = np.repeat(np.stack([tau_c, omega_c, g_c], axis=1)[:, None, :], m, axis=1)
        return knots, np.ascontiguousarray(optics)

    entries = {"shortwave (lbl_path_two_stream)": shortwave,
               "longwave, level-temperature source": longwave(False),
               "longwave, linear-in-tau source": longwave(True)}
    lines = ["scripts/scatterer_spectral_timing.py on one MI355X: %d levels x %d points, one "
             "path, upward and downward fluxes on the grid." % (levels, grid.size),
             "Times in ms: minimum (median, maximum) of %d synchronous calls that take turns, after "
             "one round that does not count;" % ROUNDS,
             "ratio: the minimum over the grey entry's.  The spectral tables are flat: every call "
             "of a block computes the same fluxes.", ""]
    for entry, make in entries.items():
        for atmosphere, (tau_c, omega_c, g_c) in scatterers.items():
            calls = {"grey entry": make(tau_c, omega_c, g_c, None)}
            for m in KNOT_COUNTS:
                calls["spectral entry, M = %d" % m] = make(tau_c, omega_c, g_c, m)
            times = {label: [] for label in calls}
            for round_ in range(ROUNDS + 1):
                for label, call in calls.items():
                    start = time.perf_counter()
                    call()
                    if round_ > 0:
                        times[label].append((time.perf_counter() - start)*1e3)
            lines.append("%s, %s" % (entry, atmosphere))
            grey = min(times["grey entry"])
            for label, values in times.items():
                lines.append("  %-28s%8.3f (%.3f, %.3f)   ratio %.3f" % (
                    label, min(values), float(np.median(values)), max(values), min(values)/grey))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    engine.free_grid(handle)
    for block in (beta, solar, sigma, work, up, down, top_up, top_down):
        engine.blocks.give(block)


if __name__ == "__main__":
    main()
