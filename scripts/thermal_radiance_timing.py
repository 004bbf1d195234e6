"""Spectroscopy.compute_thermal_radiance at the configs[3] shape on one GPU: 64-level standard
atmosphere, synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB
"total" block), a black surface, D = 1.66, a nadir view, all-clear and with a grey cloud in four
levels.

Reports, interleaved in one session (minimum and mean of ten after one call that does not count)
  * the thermal two-stream entry alone on a resident 64-level block of the real "total"
    absorption, synchronous, as scripts/thermal_flux_timing.py runs it (four row blocks with 1 cm-1
    band means: its number there is the one to compare with) and as compute_thermal_radiance
    queues it (the two flux rows per level, nothing else);
  * the radiance entry alone on the flux rows that call left (thermal_view_kernel), clear and
    cloudy, against its traffic model (beta and, in a cloudy level, two flux rows per element);
  * the pair of entries, one behind the other;
  * the wall time of compute_thermal_radiance(band_edges=1 cm-1 bins), clear and cloudy, beside
    compute_thermal_flux with the same bands.

    python scripts/thermal_radiance_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/thermal_radiance_timing.py
"""
import numpy as np

from solar_flux_timing import cloud
from solar_timing import interleaved
from timing_common import SURFACE, parser, resident_total, setup, write_report

from pylbl_amd.mt_ckd import resident_grid
from pylbl_amd.paths import DIFFUSIVITY

SWEEP_RATE = 6.3e12         # bytes/s of in-order sweeps


def main():
    args = parser(__doc__).parse_args()
    spec, grid, thickness, temperature, edges, starts, report = setup(args.levels)
    levels, bands = args.levels, edges.size - 1
    tau_c, omega_c, g_c = cloud(levels)
    zeros = np.zeros(levels)
    tables = {"clear": np.stack([thickness, zeros, zeros, zeros, temperature], axis=1),
              "cloud": np.stack([thickness, tau_c, omega_c*tau_c, g_c, temperature], axis=1)}
    tables = {name: np.ascontiguousarray(table) for name, table in tables.items()}

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    work = engine.blocks.take(2*levels, n)
    up, down = engine.blocks.take(levels, n), engine.blocks.take(levels, n)
    top_up, top_down = engine.blocks.take(1, n), engine.blocks.take(1, n)
    up_mean, down_mean = engine.blocks.take(levels, bands), engine.blocks.take(levels, bands)
    top_up_mean, top_down_mean = engine.blocks.take(1, bands), engine.blocks.take(1, bands)
    radiance = engine.blocks.take(1, n)
    everything = dict(up_rows=up, down_rows=down, top_up_rows=top_up, top_down_rows=top_down,
                      up_mean=up_mean, down_mean=down_mean, top_up_mean=top_up_mean,
                      top_down_mean=top_down_mean, band_start=starts)
    surface = dict(diffusivity=DIFFUSIVITY, emissivity=[1.], from_last=True)

    def fluxes(name, **outputs):
        return lambda: engine.path_thermal_two_stream(
            beta, grid.size, handle, 1, levels, 0, tables[name], [SURFACE], work, **surface,
            **outputs)

    def view(name):
        return lambda: engine.path_thermal_radiance(
            beta, grid.size, handle, 1, levels, 0, tables[name], [1.], [SURFACE], up, down,
            radiance_rows=radiance, **surface)

    def pair(name):
        first, second = fluxes(name, up_rows=up, down_rows=down), view(name)

        def both():
            first()
            second()
        return both

    for name in ("clear", "cloud"):
        # The radiance entry reads the flux rows of its own table: they are left by the two-stream
        # call that the interleaved loop runs just before it.
        calls = {f"path_thermal_{name}_with_means": fluxes(name, **everything),
                 f"path_thermal_{name}_flux_rows": fluxes(name, up_rows=up, down_rows=down),
                 f"path_thermal_radiance_{name}": view(name),
                 f"path_thermal_pair_{name}": pair(name)}
        for label, (low, mean) in interleaved(calls).items():
            report[f"sweep_{label}_min_ms"], report[f"sweep_{label}_mean_ms"] = low, mean
        cloudy = 0 if name == "clear" else int(np.count_nonzero(tables[name][:, 2]))
        model = (levels + 2*cloudy + 1)*grid.size*8
        report[f"path_thermal_radiance_{name}_model_ms"] = 1e3*model/SWEEP_RATE
        report[f"path_thermal_radiance_{name}_over_model"] = \
            report[f"sweep_path_thermal_radiance_{name}_min_ms"] / \
            report[f"path_thermal_radiance_{name}_model_ms"]
        report[f"path_thermal_pair_{name}_over_flux_rows"] = \
            report[f"sweep_path_thermal_pair_{name}_min_ms"] / \
            report[f"sweep_path_thermal_{name}_flux_rows_min_ms"]
    report["path_thermal_radiance_issue_model_ms"] = 1e3*(3*levels*grid.size*8)/SWEEP_RATE
    for block in (beta, work, up, down, top_up, top_down, up_mean, down_mean, top_up_mean,
                  top_down_mean, radiance):
        engine.blocks.give(block)

    # End to end with 1 cm-1 bands.
    scatterers = dict(scatterer_optical_depth=tau_c, scatterer_single_scattering_albedo=omega_c,
                      scatterer_asymmetry=g_c)
    calls = {
        "compute_thermal_flux_clear": lambda: spec.compute_thermal_flux(
            thickness, SURFACE, band_edges=edges),
        "compute_thermal_radiance_clear": lambda: spec.compute_thermal_radiance(
            thickness, SURFACE, band_edges=edges),
        "compute_thermal_flux_cloud": lambda: spec.compute_thermal_flux(
            thickness, SURFACE, band_edges=edges, **scatterers),
        "compute_thermal_radiance_cloud": lambda: spec.compute_thermal_radiance(
            thickness, SURFACE, band_edges=edges, **scatterers),
    }
    for label, (low, mean) in interleaved(calls, count=5).items():
        report[f"{label}_min_ms"], report[f"{label}_mean_ms"] = low, mean
    for name in ("clear", "cloud"):
        report[f"compute_thermal_radiance_{name}_over_compute_thermal_flux"] = \
            report[f"compute_thermal_radiance_{name}_min_ms"] / \
            report[f"compute_thermal_flux_{name}_min_ms"]
    write_report(report, args.out)


if __name__ == "__main__":
    main()
