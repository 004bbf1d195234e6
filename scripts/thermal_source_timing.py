"""Spectroscopy.compute_thermal_flux_linear at the configs[3] shape on one GPU: 64-level standard
atmosphere, synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB
"total" block), a black surface, D = 1.66, all-clear and with a grey cloud in four levels; the
interface temperatures are the means of the neighbouring levels, the outer ones the outer levels'.

Reports, interleaved in one session (minimum and mean of ten after one call that does not count)
  * the entry with the linear-in-tau source alone on a resident 64-level block of the real "total"
    absorption, synchronous, upward and downward fluxes with 1 cm-1 band means (its two kernels, up
    then down), all-clear and with the cloud, beside the isothermal entry
    Engine.path_thermal_two_stream on the same block, and their ratios;
  * the wall time of compute_thermal_flux_linear(band_edges=1 cm-1 bins), clear and cloudy, beside
    compute_thermal_flux with the same bands.

    python scripts/thermal_source_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/thermal_source_timing.py
"""
import numpy as np

from solar_flux_timing import cloud
from solar_timing import interleaved
from timing_common import SURFACE, parser, resident_total, setup, write_report

from pylbl_amd.mt_ckd import resident_grid
from pylbl_amd.paths import DIFFUSIVITY


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
    interfaces = np.concatenate([temperature[:1], (temperature[:-1] + temperature[1:])/2.,
                                 temperature[-1:]])
    edge_table = np.ascontiguousarray(np.stack([interfaces[:-1], interfaces[1:]], axis=1))

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    work = engine.blocks.take(2*levels, n)
    up, down = engine.blocks.take(levels, n), engine.blocks.take(levels, n)
    top_up, top_down = engine.blocks.take(1, n), engine.blocks.take(1, n)
    up_mean, down_mean = engine.blocks.take(levels, bands), engine.blocks.take(levels, bands)
    top_up_mean, top_down_mean = engine.blocks.take(1, bands), engine.blocks.take(1, bands)
    outputs = dict(up_rows=up, down_rows=down, top_up_rows=top_up, top_down_rows=top_down,
                   up_mean=up_mean, down_mean=down_mean, top_up_mean=top_up_mean,
                   top_down_mean=top_down_mean)
    common = dict(diffusivity=DIFFUSIVITY, emissivity=[1.], band_start=starts, from_last=True)

    def isothermal(name):
        return lambda: engine.path_thermal_two_stream(
            beta, grid.size, handle, 1, levels, 0, tables[name], [SURFACE], work, **common,
            **outputs)

    def linear(name):
        return lambda: engine.path_thermal_two_stream_source(
            beta, grid.size, handle, 1, levels, 0, tables[name], edge_table, [SURFACE], work,
            **common, **outputs)
    for label, (low, mean) in interleaved({"path_thermal_clear": isothermal("clear"),
                                           "path_thermal_source_clear": linear("clear"),
                                           "path_thermal_cloud": isothermal("cloud"),
                                           "path_thermal_source_cloud": linear("cloud")}).items():
        report[f"sweep_{label}_min_ms"], report[f"sweep_{label}_mean_ms"] = low, mean
    for name in ("clear", "cloud"):
        report[f"path_thermal_source_{name}_over_path_thermal_{name}"] = \
            report[f"sweep_path_thermal_source_{name}_min_ms"] / \
            report[f"sweep_path_thermal_{name}_min_ms"]
    for block in (beta, work, up, down, top_up, top_down, up_mean, down_mean, top_up_mean,
                  top_down_mean):
        engine.blocks.give(block)

    # End to end with 1 cm-1 bands.
    scatterers = dict(scatterer_optical_depth=tau_c, scatterer_single_scattering_albedo=omega_c,
                      scatterer_asymmetry=g_c)
    calls = {
        "compute_thermal_flux_clear": lambda: spec.compute_thermal_flux(
            thickness, SURFACE, band_edges=edges),
        "compute_thermal_flux_linear_clear": lambda: spec.compute_thermal_flux_linear(
            thickness, SURFACE, interfaces, band_edges=edges),
        "compute_thermal_flux_cloud": lambda: spec.compute_thermal_flux(
            thickness, SURFACE, band_edges=edges, **scatterers),
        "compute_thermal_flux_linear_cloud": lambda: spec.compute_thermal_flux_linear(
            thickness, SURFACE, interfaces, band_edges=edges, **scatterers),
    }
    for label, (low, mean) in interleaved(calls, count=5).items():
        report[f"{label}_min_ms"], report[f"{label}_mean_ms"] = low, mean
    for name in ("clear", "cloud"):
        report[f"compute_thermal_flux_linear_{name}_over_compute_thermal_flux"] = \
            report[f"compute_thermal_flux_linear_{name}_min_ms"] / \
            report[f"compute_thermal_flux_{name}_min_ms"]
    write_report(report, args.out)


if __name__ == "__main__":
    main()
