"""Spectroscopy.compute_jacobian at the configs[3] shape on one GPU: 64-level standard atmosphere,
synthetic H2O, CO2 and O3 tables, 1-3000 cm-1 at 0.001 cm-1 (3 M points, a 1.5 GB "total" block),
radiance plus the optical-depth and temperature Jacobians.

Reports
  * path_jacobian_kernel alone (Engine.path_jacobian on a resident 64-level block of the real
    "total" absorption, synchronous, best of ten) beside the cumulative optical-depth sweep
    (Engine.path_compute) and the radiance sweep (Engine.path_radiance) on the same block, the
    bytes it moves (beta twice, W written and read, one block per per-level Jacobian) and those
    as a fraction of 6.3 TB/s;
  * the wall time of compute_jacobian(instrument=X) beside compute_radiance(instrument=X,
    cumulative=True), X the IASI-like Gaussian of scripts/instrument_timing.py (median of three
    after a warm-up);
  * the channel Jacobian dR_c/dln x_k of the path by 65 compute_radiance(instrument=X) calls with
    perturbed path lengths (one-sided, step 1e-4) beside the one compute_jacobian call: both
    times and the largest difference relative to the largest |dR_c/dln x| of the channel;
  * the largest deviation of the GPU result from the numpy mirror (tests/jacobian_cases.py,
    float64) on every 16th column of the block, in units of 1e-12 times the magnitude each
    quantity is formed from.

    python scripts/jacobian_timing.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/jacobian_timing.py --kernels-only
"""
import time

import numpy as np

from timing_common import PEAK, SURFACE, best_of, iasi_like, median_wall, parser, \
    resident_total, setup, write_report

from pylbl_amd.mt_ckd import resident_grid


def main():
    arguments = parser(__doc__)
    arguments.add_argument("--kernels-only", action="store_true",
                           help="the sweeps on the resident block alone (for a kernel trace)")
    args = arguments.parse_args()
    spec, grid, lengths, temperature, _, _, report = setup(args.levels)
    surface = SURFACE
    levels = args.levels

    engine, beta, n = resident_total(spec)
    handle = resident_grid(engine, spec.grid)
    carry, rad = engine.blocks.take(1, n), engine.blocks.take(1, n)
    work, depth, dtemp = (engine.blocks.take(levels, n) for _ in range(3))
    common = (beta, grid.size, handle, 1, levels, 0, lengths, temperature)
    sweeps = {
        # (call, row streams of [levels, points] moved)
        "tau_cumulative": (lambda: engine.path_compute(
            beta, grid.size, 1, levels, 0, lengths, carry, optical_depth=depth,
            cumulative=True), 2),
        "radiance": (lambda: engine.path_radiance(
            *common, carry, boundary_temperature=[surface], radiance=rad), 1),
        "jacobian": (lambda: engine.path_jacobian(
            *common, work, boundary_temperature=[surface], radiance=rad,
            optical_depth_jacobian=depth, temperature_jacobian=dtemp), 6),
        "jacobian_in_place": (lambda: engine.path_jacobian(
            *common, work, boundary_temperature=[surface], radiance=rad,
            optical_depth_jacobian=work, temperature_jacobian=dtemp), 6),
        "jacobian_depth_only": (lambda: engine.path_jacobian(
            *common, work, boundary_temperature=[surface], optical_depth_jacobian=depth), 5),
    }
    block_bytes = levels*grid.size*8
    report["block_bytes"] = block_bytes
    for label, (sweep, streams) in sweeps.items():
        best = best_of(sweep)
        report[f"sweep_{label}_ms"] = best*1e3
        report[f"sweep_{label}_bytes"] = streams*block_bytes
        report[f"sweep_{label}_fraction_of_6.3TBps"] = streams*block_bytes/best/PEAK
    if args.kernels_only:
        write_report(report)
        return

    # The GPU against the float64 numpy mirror, on every 16th column.
    from tests import jacobian_cases as jac
    sweeps["jacobian"][0]()
    columns = np.arange(0, grid.size, 16)
    beta_host = beta.to_host()[:, :grid.size][:, columns]
    values, magnitudes = jac.jacobian(np.float64, grid[columns], beta_host, lengths, temperature,
                                      levels, False, np.array([surface]), np.array([1.]))
    for q, block in (("radiance", rad), ("optical_depth_jacobian", depth),
                     ("temperature_jacobian", dtemp)):
        got = block.to_host()[:, :grid.size][:, columns]
        allowed = 1e-12*magnitudes[q]
        error = np.abs(got - values[q])
        report[f"{q}_max_error_over_1e-12_magnitude"] = float(
            np.max(error[allowed > 0.]/allowed[allowed > 0.]))
    del beta_host
    for block in (beta, carry, rad, work, depth, dtemp):
        engine.blocks.give(block)

    # End to end with the IASI-like instrument.
    instrument = iasi_like()
    report["channels"] = len(instrument)
    quantities = ("radiance", "optical_depth_jacobian", "temperature_jacobian")
    report["compute_jacobian_instrument_ms"] = 1e3*median_wall(lambda: spec.compute_jacobian(
        lengths, boundary_temperature=surface, instrument=instrument, quantities=quantities))
    report["compute_radiance_instrument_cumulative_ms"] = 1e3*median_wall(
        lambda: spec.compute_radiance(lengths, boundary_temperature=surface,
                                      instrument=instrument, cumulative=True))
    report["compute_jacobian_over_cumulative_radiance"] = \
        report["compute_jacobian_instrument_ms"]/report["compute_radiance_instrument_cumulative_ms"]

    # What users do today: L + 1 radiance calls with perturbed path lengths.
    d = 1e-4
    start = time.perf_counter()
    base = np.asarray(spec.compute_radiance(lengths, boundary_temperature=surface,
                                            instrument=instrument)["radiance"])
    differences = np.zeros((levels, len(instrument)))
    for level in range(levels):
        s = lengths.copy()
        s[level] *= 1. + d
        moved = np.asarray(spec.compute_radiance(s, boundary_temperature=surface,
                                                 instrument=instrument)["radiance"])
        differences[level] = (moved - base)/d
    report["finite_difference_calls"] = levels + 1
    report["finite_difference_ms"] = 1e3*(time.perf_counter() - start)
    start = time.perf_counter()
    analytic = np.asarray(spec.compute_jacobian(
        lengths, boundary_temperature=surface, instrument=instrument,
        quantities="log_optical_depth_jacobian")["log_optical_depth_jacobian"])
    report["analytic_ms"] = 1e3*(time.perf_counter() - start)
    scale = np.nanmax(np.abs(analytic), axis=0)
    report["finite_difference_max_difference_of_channel_max"] = float(
        np.nanmax(np.abs(differences - analytic)/scale))
    write_report(report, args.out)


if __name__ == "__main__":
    main()
