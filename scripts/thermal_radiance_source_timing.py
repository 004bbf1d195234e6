"""lbl_path_thermal_radiance_source beside lbl_path_thermal_radiance at the configs[3] shape on one
GPU: 64-level standard atmosphere, synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M
points, a 1.5 GB "total" block), a black surface, D = 1.66, a nadir view, all-clear and with a grey
cloud in four levels; the interface temperatures are the means of the neighbouring level
temperatures, the outermost two the level's own.

Reports, interleaved in one session (minimum and mean of ten after one round that does not count)
on a resident 64-level block of the real "total" absorption, synchronous
  * the two flux entries as the radiance calls queue them (the two flux rows per level, nothing
    else): lbl_path_thermal_two_stream and lbl_path_thermal_two_stream_source;
  * the two view entries alone, each on the flux rows its own flux entry left just before it:
    lbl_path_thermal_radiance (thermal_view_kernel) and lbl_path_thermal_radiance_source
    (thermal_view_source_kernel);
  * the two pairs, one entry behind the other;
  * the ratios source / isothermal of each.
The untouched grey view entry is compared between two commits with
scripts/thermal_radiance_timing.py, run from a checkout of each in turn in one session.

    python scripts/thermal_radiance_source_timing.py [--out FILE]
"""
import numpy as np

from solar_flux_timing import cloud
from solar_timing import interleaved
from timing_common import SURFACE, parser, resident_total, setup, write_report

from pylbl_amd.mt_ckd import resident_grid
from pylbl_amd.paths import DIFFUSIVITY


def edge_table(temperature):
    """[levels, 2]: the interface temperatures of each level on its first-level and last-level
    side, the mean of the two levels an interface lies between."""
    inner = (temperature[:-1] + temperature[1:])/2.
    interfaces = np.concatenate([temperature[:1], inner, temperature[-1:]])
    return np.ascontiguousarray(np.stack([interfaces[:-1], interfaces[1:]], axis=1))


def main():
    args = parser(__doc__).parse_args()
    spec, grid, thickness, temperature, edges, starts, report = setup(args.levels)
    levels = args.levels
    tau_c, omega_c, g_c = cloud(levels)
    zeros = np.zeros(levels)
    tables = {"clear": np.stack([thickness, zeros, zeros, zeros, temperature], axis=1),
              "cloud": np.stack([thickness, tau_c, omega_c*tau_c, g_c, temperature], axis=1)}
    tables = {name: np.ascontiguousarray(table) for name, table in tables.items()}
    faces = edge_table(temperature)

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    work = engine.blocks.take(2*levels, n)
    up, down = engine.blocks.take(levels, n), engine.blocks.take(levels, n)
    radiance = engine.blocks.take(1, n)
    surface = dict(diffusivity=DIFFUSIVITY, emissivity=[1.], from_last=True)
    run = (beta, grid.size, handle, 1, levels, 0)

    def fluxes(name, linear):
        if linear:
            return lambda: engine.path_thermal_two_stream_source(
                *run, tables[name], faces, [SURFACE], work, up_rows=up, down_rows=down, **surface)
        return lambda: engine.path_thermal_two_stream(
            *run, tables[name], [SURFACE], work, up_rows=up, down_rows=down, **surface)

    def view(name, linear):
        if linear:
            return lambda: engine.path_thermal_radiance_source(
                *run, tables[name], faces, [1.], [SURFACE], up, down, radiance_rows=radiance,
                **surface)
        return lambda: engine.path_thermal_radiance(
            *run, tables[name], [1.], [SURFACE], up, down, radiance_rows=radiance, **surface)

    def pair(name, linear):
        first, second = fluxes(name, linear), view(name, linear)

        def both():
            first()
            second()
        return both

    sources = {"isothermal": False, "source": True}
    for name in ("clear", "cloud"):
        # A view entry reads the flux rows of its own table and source: they are left by the flux
        # entry that the interleaved loop runs just before it.
        calls = {}
        for source, linear in sources.items():
            calls[f"flux_{source}_{name}"] = fluxes(name, linear)
            calls[f"view_{source}_{name}"] = view(name, linear)
        for source, linear in sources.items():
            calls[f"pair_{source}_{name}"] = pair(name, linear)
        for label, (low, mean) in interleaved(calls).items():
            report[f"{label}_min_ms"], report[f"{label}_mean_ms"] = low, mean
        for what in ("flux", "view", "pair"):
            for kind in ("min", "mean"):
                report[f"{what}_{name}_source_over_isothermal_{kind}"] = \
                    report[f"{what}_source_{name}_{kind}_ms"] / \
                    report[f"{what}_isothermal_{name}_{kind}_ms"]
    for block in (beta, work, up, down, radiance):
        engine.blocks.give(block)
    del edges, starts
    write_report(report, args.out)


if __name__ == "__main__":
    main()
