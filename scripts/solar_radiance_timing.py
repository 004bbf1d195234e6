"""Spectroscopy.compute_solar_radiance at the configs[3] shape on one GPU: 64-level standard
atmosphere, synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB
"total" block), the Sun at mu0 = 0.5 over a surface of albedo 0.3, a view along mu = 0.8 at phi =
140 degrees, in three cases: clear without Rayleigh scattering, Rayleigh scattering only, Rayleigh
scattering and scripts/solar_flux_timing.py's grey cloud in four levels.

Expected traffic, written down before the first run: the view kernel reads beta and, in a level
that scatters, three flux rows per level and element, and writes one row per path: (64 + 1) rows
without scattering, (4*64 + 1) rows where every level scatters, 8 bytes each -- 1.56 GB and 6.17
GB, 0.25 ms and 0.98 ms at the 6.3 TB/s of in-order sweeps.

Reports, interleaved in one session (minimum and mean of ten after one call that does not count),
per case
  * the two-stream entry alone on a resident 64-level block of the real "total" absorption,
    synchronous, as compute_solar_radiance queues it (the three flux rows per level, nothing
    else);
  * the radiance entry alone on the flux rows that call left (solar_view_kernel), against the
    traffic above;
  * the pair of entries, one behind the other, and its ratio to the two-stream entry alone.

    python scripts/solar_radiance_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/solar_radiance_timing.py
"""
import numpy as np

from solar_flux_timing import ALBEDO, MU0, cloud
from solar_timing import interleaved
from timing_common import parser, resident_total, setup, write_report

from pylbl_amd.mt_ckd import resident_grid
from pylbl_amd.paths import K_B, SOLAR_SOLID_ANGLE, SOLAR_TEMPERATURE

SWEEP_RATE = 6.3e12         # bytes/s of in-order sweeps
MU, PHI = 0.8, 140.


def main():
    args = parser(__doc__).parse_args()
    spec, grid, thickness, temperature, edges, starts, report = setup(args.levels)
    levels = args.levels
    tau_c, omega_c, g_c = cloud(levels)
    air = (np.asarray(spec.atmosphere.pressure, dtype=np.float64).ravel() /
           (K_B*temperature))*thickness
    w_c = omega_c*tau_c
    zeros = np.zeros(levels)
    tables = {"clear": np.stack([thickness, zeros, zeros, zeros, zeros], axis=1),
              "rayleigh": np.stack([thickness, air, zeros, zeros, zeros], axis=1),
              "cloud": np.stack([thickness, air, tau_c, w_c, w_c*g_c], axis=1)}
    tables = {name: np.ascontiguousarray(table) for name, table in tables.items()}
    cos_theta = -MU*MU0 + (np.sqrt((1. - MU)*(1. + MU))*np.sqrt((1. - MU0)*(1. + MU0))) * \
        np.cos(PHI*np.pi/180.)

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    solar, sigma = engine.blocks.take(1, n), engine.blocks.take(1, n)
    work = engine.blocks.take(2*levels, n)
    up, direct, diffuse = (engine.blocks.take(levels, n) for _ in range(3))
    radiance = engine.blocks.take(1, n)
    engine.solar_spectrum(handle, solar, grid.size, temperature=SOLAR_TEMPERATURE,
                          scale=SOLAR_SOLID_ANGLE)
    engine.rayleigh_row(handle, sigma, grid.size)
    rows = dict(up_rows=up, direct_rows=direct, diffuse_rows=diffuse)

    def surface(name):
        return dict(rayleigh_row=None if name == "clear" else sigma, albedo=[ALBEDO],
                    from_last=True)

    def fluxes(name):
        return lambda: engine.path_two_stream(
            beta, grid.size, 1, levels, 0, tables[name], [MU0], solar, work, **surface(name),
            **rows)

    def view(name):
        return lambda: engine.path_solar_radiance(
            beta, grid.size, 1, levels, 0, tables[name], [MU0], [MU], [cos_theta], solar,
            radiance_rows=radiance, **surface(name), **rows)

    def pair(name):
        first, second = fluxes(name), view(name)

        def both():
            first()
            second()
        return both

    for name in tables:
        # The radiance entry reads the flux rows of its own table: they are left by the two-stream
        # call that the interleaved loop runs just before it.
        calls = {f"path_two_stream_{name}_flux_rows": fluxes(name),
                 f"path_solar_radiance_{name}": view(name),
                 f"path_solar_pair_{name}": pair(name)}
        for label, (low, mean) in interleaved(calls).items():
            report[f"sweep_{label}_min_ms"], report[f"sweep_{label}_mean_ms"] = low, mean
        scattering = 0 if name == "clear" else levels
        model = (levels + 3*scattering + 1)*grid.size*8
        report[f"path_solar_radiance_{name}_model_ms"] = 1e3*model/SWEEP_RATE
        report[f"path_solar_radiance_{name}_over_model"] = \
            report[f"sweep_path_solar_radiance_{name}_min_ms"] / \
            report[f"path_solar_radiance_{name}_model_ms"]
        report[f"path_solar_pair_{name}_over_flux_rows"] = \
            report[f"sweep_path_solar_pair_{name}_min_ms"] / \
            report[f"sweep_path_two_stream_{name}_flux_rows_min_ms"]
        report[f"path_solar_radiance_{name}_per_level_ms"] = \
            report[f"sweep_path_solar_radiance_{name}_min_ms"]/levels
    for block in (beta, solar, sigma, work, up, direct, diffuse, radiance):
        engine.blocks.give(block)
    write_report(report, args.out)


if __name__ == "__main__":
    main()
