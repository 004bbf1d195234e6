"""Spectroscopy.compute_thermal_flux at the configs[3] shape on one GPU: 64-level standard
atmosphere, synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB
"total" block), a black surface, D = 1.66, all-clear and with a grey cloud in four levels.

Reports, interleaved in one session (minimum and mean of ten after one call that does not count)
  * the thermal two-stream entry alone on a resident 64-level block of the real "total"
    absorption, synchronous, upward and downward fluxes with 1 cm-1 band means (its two kernels, up
    then down), all-clear and with the cloud, beside Engine.path_flux with one angle, down pass and
    up pass (path_flux_kernel<., 1> twice), and the shortwave entry Engine.path_two_stream with the
    same cloud;
  * the wall time of compute_thermal_flux(band_edges=1 cm-1 bins), clear and cloudy, beside
    compute_flux(angles=1) with the same bands.

    python scripts/thermal_flux_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/thermal_flux_timing.py
"""
import numpy as np

from solar_flux_timing import ALBEDO, MU0, cloud
from solar_timing import interleaved
from timing_common import SURFACE, parser, resident_total, setup, write_report

from pylbl_amd.mt_ckd import resident_grid
from pylbl_amd.paths import DIFFUSIVITY, K_B, SOLAR_SOLID_ANGLE, SOLAR_TEMPERATURE


def main():
    args = parser(__doc__).parse_args()
    spec, grid, thickness, temperature, edges, starts, report = setup(args.levels)
    levels, bands = args.levels, edges.size - 1
    tau_c, omega_c, g_c = cloud(levels)
    zeros = np.zeros(levels)
    w_c = omega_c*tau_c
    tables = {"clear": np.stack([thickness, zeros, zeros, zeros, temperature], axis=1),
              "cloud": np.stack([thickness, tau_c, w_c, g_c, temperature], axis=1)}
    tables = {name: np.ascontiguousarray(table) for name, table in tables.items()}
    air = (np.asarray(spec.atmosphere.pressure, dtype=np.float64).ravel() /
           (K_B*temperature))*thickness
    shortwave = np.ascontiguousarray(np.stack([thickness, air, tau_c, w_c, w_c*g_c], axis=1))

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    solar, sigma = engine.blocks.take(1, n), engine.blocks.take(1, n)
    work = engine.blocks.take(2*levels, n)
    up, down = engine.blocks.take(levels, n), engine.blocks.take(levels, n)
    top_up, top_down = engine.blocks.take(1, n), engine.blocks.take(1, n)
    up_mean, down_mean = engine.blocks.take(levels, bands), engine.blocks.take(levels, bands)
    top_up_mean, top_down_mean = engine.blocks.take(1, bands), engine.blocks.take(1, bands)
    carry, reflection = engine.blocks.take(1, n), engine.blocks.take(1, n)
    engine.solar_spectrum(handle, solar, grid.size, temperature=SOLAR_TEMPERATURE,
                          scale=SOLAR_SOLID_ANGLE)
    engine.rayleigh_row(handle, sigma, grid.size)
    outputs = dict(up_rows=up, down_rows=down, top_up_rows=top_up, top_down_rows=top_down,
                   up_mean=up_mean, down_mean=down_mean, top_up_mean=top_up_mean,
                   top_down_mean=top_down_mean)

    def thermal(name):
        return lambda: engine.path_thermal_two_stream(
            beta, grid.size, handle, 1, levels, 0, tables[name], [SURFACE], work,
            diffusivity=DIFFUSIVITY, emissivity=[1.], band_start=starts, from_last=True,
            **outputs)

    def two_stream():
        engine.path_two_stream(
            beta, grid.size, 1, levels, 0, shortwave, [MU0], solar, work, rayleigh_row=sigma,
            albedo=[ALBEDO], band_start=starts, from_last=True, **outputs)

    lengths = thickness[:, None]*DIFFUSIVITY

    def flux(is_up):
        return lambda: engine.path_flux(
            beta, grid.size, handle, 1, levels, 0, lengths, [1.], temperature, carry, reflection,
            up if is_up else down, surface_temperature=[SURFACE], surface_emissivity=[1.],
            flux=up_mean if is_up else down_mean,
            surface_flux=top_up_mean if is_up else None, band_start=starts, up=is_up,
            from_last=not is_up)
    for label, (low, mean) in interleaved({"path_thermal_clear": thermal("clear"),
                                           "path_thermal_cloud": thermal("cloud"),
                                           "path_two_stream": two_stream,
                                           "path_flux_down": flux(False),
                                           "path_flux_up": flux(True)}).items():
        report[f"sweep_{label}_min_ms"], report[f"sweep_{label}_mean_ms"] = low, mean
    both = report["sweep_path_flux_down_min_ms"] + report["sweep_path_flux_up_min_ms"]
    for name in ("path_thermal_clear", "path_thermal_cloud", "path_two_stream"):
        report[f"{name}_over_path_flux_both"] = report[f"sweep_{name}_min_ms"]/both
    for block in (beta, solar, sigma, work, up, down, top_up, top_down, up_mean, down_mean,
                  top_up_mean, top_down_mean, carry, reflection):
        engine.blocks.give(block)

    # End to end with 1 cm-1 bands.
    calls = {
        "compute_flux_one_angle": lambda: spec.compute_flux(
            thickness, SURFACE, angles=1, band_edges=edges),
        "compute_thermal_flux_clear": lambda: spec.compute_thermal_flux(
            thickness, SURFACE, band_edges=edges),
        "compute_thermal_flux_cloud": lambda: spec.compute_thermal_flux(
            thickness, SURFACE, scatterer_optical_depth=tau_c,
            scatterer_single_scattering_albedo=omega_c, scatterer_asymmetry=g_c,
            band_edges=edges),
    }
    for label, (low, mean) in interleaved(calls, count=5).items():
        report[f"{label}_min_ms"], report[f"{label}_mean_ms"] = low, mean
    for name in ("clear", "cloud"):
        report[f"compute_thermal_flux_{name}_over_compute_flux"] = \
            report[f"compute_thermal_flux_{name}_min_ms"]/report["compute_flux_one_angle_min_ms"]
    write_report(report, args.out)


if __name__ == "__main__":
    main()
