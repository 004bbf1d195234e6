"""CPU checks behind tests/test_gpu_sweep_shapes.py: the long-double references of
tests/sweep_cases.py agree with the float64 numpy loops of the existing sweep tests, its mirrors of
the host and lane arithmetic restate the constants of csrc/path.h and csrc/flux.h, and the case
tables reach, through those mirrors, every instantiation of the three sweep kernels, every loop of
path_levels with every (starts, finishes) pair, and every band-segment edge."""
from pathlib import Path
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import sweep_cases as cases

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pylbl_amd" / "csrc"
F64, LD = np.float64, np.longdouble


def constant(text, name):
    return re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text).group(1).strip()


def test_constants_match_the_headers():
    path, flux = (CSRC / "path.h").read_text(), (CSRC / "flux.h").read_text()
    assert int(constant(path, "kPathThreads")) == cases.PATH_THREADS
    assert int(constant(path, "kPathWidth")) == cases.PATH_WIDTH
    assert int(constant(path, "kPathAhead")) == cases.PATH_AHEAD
    assert int(constant(path, "kPathSegment")) == cases.PATH_SEGMENT
    assert int(constant(flux, "kFluxMaxAngles")) == cases.FLUX_MAX_ANGLES
    assert float(constant(flux, "kFluxPi")) == cases.FLUX_PI == np.pi
    assert constant(flux, "kFluxAhead") == "K <= %d ? kPathAhead : %d" % (
        cases.FLUX_AHEAD_SPLIT, cases.FLUX_AHEAD_MANY)
    assert [cases.flux_ahead(k) for k in range(1, 9)] == [8, 8, 8, 8, 4, 4, 4, 4]
    # the long-double references need more than float64: x86 extended
    assert np.finfo(LD).eps < 2.e-19


def test_mirrors_on_known_answers():
    assert cases.path_vector(10, [0, 0]) and not cases.path_vector(11, [0])
    assert not cases.path_vector(10, [0, 1])
    assert cases.lane_widths(1) == {1} and cases.lane_widths(512) == {2}
    assert cases.lane_widths(513) == {1, 2}
    assert cases.path_lanes(11, 38, 19, False) == [
        cases.Lane(0, 8, False, True), cases.Lane(1, 19, True, True),
        cases.Lane(2, 11, True, False)]
    assert cases.path_lanes(11, 38, 19, True) == [
        cases.Lane(0, 8, True, False), cases.Lane(1, 19, True, True),
        cases.Lane(2, 11, False, True)]
    assert cases.batches(19, 8) == (2, 3) and cases.batches(11, 4) == (2, 3)
    assert cases.band_segments([0, 0, 4000, 8193]) == [
        (1, 0, 4000), (2, 4000, 4096), (2, 4096, 8192), (2, 8192, 8193)]
    assert cases.run_sets(19)["uneven"] == [(0, 11), (11, 38), (49, 8)]
    for n in cases.LEVELS + cases.LEVELS_MANY:
        for name, runs in cases.run_sets(n).items():
            # the runs tile the flat levels in order
            assert runs[0][0] == 0 and sum(c for _, c in runs) == cases.PATHS*n, name
            assert all(a + c == b for (a, c), (b, _) in zip(runs, runs[1:])), name


# ---------------------------------------------------------------------------------------------
# The references against the float64 loops of the existing tests.
def positive_problem():
    return cases.Problem(1031, 43//cases.PATHS + 1, seed=5)


def worst_relative(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    scale = np.maximum(np.abs(b), LD(1e-300))
    return float(np.max(np.abs(a - b)/scale))


@pytest.mark.parametrize("from_last", [False, True])
def test_references_agree_with_the_float64_loops_of_the_suite(from_last):
    """Far inside the GPU bound of 1e-12 (radiance: 3.5e-15 measured)."""
    from tests.test_gpu_path import numpy_tau
    from tests.test_gpu_radiance import numpy_radiance
    problem = positive_problem()
    n, columns = problem.levels_per_path, problem.columns
    shaped = problem.beta.reshape(cases.PATHS, n, columns)
    lengths = problem.thickness.reshape(cases.PATHS, n)
    tau, mag = cases.sweep_tau(LD, problem.beta, problem.thickness, n, from_last)
    loop = numpy_tau(shaped, lengths, "from_last" if from_last else "from_first")
    assert worst_relative(loop.reshape(-1, columns), tau) < 1e-14
    assert np.array_equal(tau, mag)         # beta >= 0: the magnitude is the value
    # the float64 form of the same function is that loop bit for bit
    mine, _ = cases.sweep_tau(F64, problem.beta, problem.thickness, n, from_last)
    assert np.array_equal(mine, loop.reshape(-1, columns))

    spec = SimpleNamespace(grid=problem.nu, atmosphere=SimpleNamespace(
        temperature=problem.temperature.reshape(cases.PATHS, n)))
    loop = numpy_radiance(spec, shaped, lengths, problem.boundary_t, problem.boundary_e,
                          direction="toward_first" if from_last else "toward_last",
                          cumulative=True)
    start = cases.boundary_start(LD, problem.nu, problem.boundary_t, problem.boundary_e)
    rad, mag = cases.sweep_radiance(LD, problem.nu, problem.beta, problem.thickness,
                                    problem.temperature, n, from_last, start)
    worst = worst_relative(loop.reshape(-1, columns), rad)
    print("radiance, float64 loop against long double: %.3g" % worst)
    assert worst < 2e-14
    assert worst_relative(mag, rad) < 1e-18
    start = cases.boundary_start(F64, problem.nu, problem.boundary_t, problem.boundary_e)
    mine, _ = cases.sweep_radiance(F64, problem.nu, problem.beta, problem.thickness,
                                   problem.temperature, n, from_last, start)
    assert np.array_equal(mine, loop.reshape(-1, columns))


@pytest.mark.parametrize("surface", ["first", "last"])
def test_flux_reference_agrees_with_the_float64_loop_of_the_suite(surface):
    from tests.test_gpu_flux import numpy_flux
    problem = cases.Problem(257, 11, seed=6)
    n, columns = problem.levels_per_path, problem.columns
    shape = (cases.PATHS, n)
    spec = SimpleNamespace(grid=problem.nu, atmosphere=SimpleNamespace(
        temperature=problem.temperature.reshape(shape), pressure=np.full(shape, 5e4)))
    thickness = problem.thickness.reshape(shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        loop = numpy_flux(spec, problem.beta.reshape(shape + (columns,)), thickness,
                          problem.surface_t, problem.surface_e, surface=surface, angles=5)
    lengths, weight = problem.lengths(5)
    down_last = surface == "first"
    down = cases.sweep_flux(LD, problem.nu, problem.beta, lengths, weight, problem.temperature, n,
                            down_last)
    start, start_mag = cases.surface_start(LD, problem.nu, problem.surface_t, problem.surface_e,
                                           down.total, down.total_mag)
    up = cases.sweep_flux(LD, problem.nu, problem.beta, lengths, weight, problem.temperature, n,
                          not down_last, start, start_mag)
    # interfaces [paths, n + 1]: with the surface first, level l's down flux is at l, its up flux
    # at l + 1, and interface 0 is the surface
    lo, hi = slice(0, n), slice(1, n + 1)
    loop_down = loop["downward_flux"][:, lo if surface == "first" else hi]
    loop_up = loop["upward_flux"][:, hi if surface == "first" else lo]
    assert worst_relative(loop_down.reshape(-1, columns), down.flux) < 2e-14
    assert worst_relative(loop_up.reshape(-1, columns), up.flux) < 2e-14
    at_surface = loop["upward_flux"][:, 0 if surface == "first" else n]
    mine = LD(cases.FLUX_PI)*cases.flux_sum(weight.astype(LD), np.repeat(
        start[:, None, :], weight.size, axis=1))
    assert worst_relative(at_surface, mine) < 2e-14
    assert worst_relative(up.flux_mag, up.flux) < 1e-18


# ---------------------------------------------------------------------------------------------
# Coverage of the case tables, through the mirrors.
def test_every_instantiation_is_selected():
    """2 + 2 + 16: {vector, scalar} x {path, radiance, flux K = 1..8}."""
    kinds = {cases.layout_is_vector(name, columns)
             for name in cases.LAYOUTS for columns in cases.LAYOUT_COLUMNS}
    assert kinds == {True, False}
    # the layouts run for every kernel on LAYOUT_COLUMNS and for every K on ANGLE_COLUMNS
    for columns in cases.LAYOUT_COLUMNS + (cases.ANGLE_COLUMNS,):
        assert cases.layout_is_vector("aligned", columns)
        assert not cases.layout_is_vector("offset", columns)
        assert not cases.layout_is_vector("odd", columns)
        assert cases.layout_is_vector("exact", columns) == (columns % 2 == 0)
        assert cases.layout_is_vector("padded", columns) == (columns % 2 == 1)
    assert cases.ANGLES == (1, 2, 3, 4, 5, 6, 7, 8)
    # a lane of width 1 in both kinds of kernel, and the padded vector layout has one too
    assert any(1 in cases.lane_widths(c) for c in cases.LAYOUT_COLUMNS)
    assert 1 in cases.lane_widths(cases.ANGLE_COLUMNS) and 1 in cases.lane_widths(cases.RUN_COLUMNS)
    assert set(cases.COLUMNS) == {1, 2, 3, 511, 512, 513, 1031, 8193}
    assert max(cases.COLUMNS) <= 8193


@pytest.mark.parametrize("from_last", [False, True])
@pytest.mark.parametrize("kernel", ["path", "radiance", "flux"])
def test_runs_reach_every_loop_of_path_levels(kernel, from_last):
    aheads = {}
    for n, angles, sets in cases.run_cases(kernel):
        ahead = cases.kernel_ahead(kernel, angles)
        seen = aheads.setdefault(ahead, {"classes": set(), "mixed": False})
        for name, runs in sets.items():
            for first, count in runs:
                lanes = cases.path_lanes(first, count, n, from_last)
                for lane in lanes:
                    full, rest = cases.batches(lane.n, ahead)
                    if full == 0:
                        depth = "n < ahead"
                    elif full == 1 and rest == 0:
                        depth = "n == ahead"
                    elif full == 1:
                        depth = "n == ahead + r"
                    elif rest > 0:
                        depth = "n >= 2 ahead + r"
                    else:
                        continue
                    seen["classes"].add((depth, lane.starts, lane.finishes))
                # the tail of one path, whole paths and the head of another in one launch
                if len(lanes) >= 3 and not (lanes[0].starts and lanes[0].finishes) and \
                        not (lanes[-1].starts and lanes[-1].finishes) and \
                        all(x.starts and x.finishes for x in lanes[1:-1]):
                    seen["mixed"] = True
    assert set(aheads) == ({8, 4} if kernel == "flux" else {8})
    for ahead, seen in aheads.items():
        expect = {(d, s, f) for d in ("n < ahead", "n == ahead", "n == ahead + r",
                                      "n >= 2 ahead + r")
                  for s in (False, True) for f in (False, True)}
        assert seen["classes"] >= expect, (ahead, sorted(expect - seen["classes"]))
        assert seen["mixed"], ahead


def test_every_angle_count_sees_full_batches_and_a_remainder():
    for angles in cases.ANGLES:
        n = cases.angle_levels(angles)
        assert n <= 19
        full, rest = cases.batches(n, cases.flux_ahead(angles))
        assert full == 2 and rest == 3
        # and across the uneven runs: a lane with a batch and a remainder that continues
        lanes = [lane for first, count in cases.run_sets(n)["uneven"]
                 for lane in cases.path_lanes(first, count, n, False)]
        assert any(cases.batches(x.n, cases.flux_ahead(angles)) >= (1, 1) and not x.finishes
                   for x in lanes)


def test_band_sets_reach_every_segment_edge():
    lengths, flags = set(), set()
    for name, columns, starts in cases.BAND_SETS:
        assert columns % 2 == 1 and starts[0] == 0 and starts[-1] == columns
        assert np.all(np.diff(starts) >= 0)
        segments = cases.band_segments(starts)
        assert all(0 < e - b <= cases.PATH_SEGMENT for _, b, e in segments)
        lengths |= {e - b for _, b, e in segments}
        per_band = [sum(1 for s in segments if s[0] == b) for b in range(len(starts) - 1)]
        for b in range(len(starts) - 1):
            lo, hi = starts[b], starts[b + 1]
            if lo == hi:
                flags.add("empty at 0" if lo == 0 else "empty at columns" if lo == columns
                          else "empty in the middle")
                continue
            if hi % cases.PATH_SEGMENT == 0 and lo % cases.PATH_SEGMENT != 0:
                flags.add("ends on a multiple of the segment")
            if lo % cases.PATH_SEGMENT == 0 and lo > 0:
                flags.add("starts on a multiple of the segment")
            if per_band[b] == 3:
                flags.add("three segments")
            if hi == columns:
                flags.add("ends at odd columns")
    assert lengths >= {1, 63, 64, 65, 4096}, lengths
    assert flags == {"empty at 0", "empty in the middle", "empty at columns",
                     "ends on a multiple of the segment", "starts on a multiple of the segment",
                     "three segments", "ends at odd columns"}, flags


# ---------------------------------------------------------------------------------------------
# The extreme-value table: no input sits on a threshold of libm or of float64's range.
def value_sweeps(kind):
    v = cases.value_problem()
    n = v.levels_per_path
    out = {}
    for from_last in (False, True):
        tau, _ = cases.sweep_tau(kind, v.beta, v.thickness, n, from_last)
        out["tau", from_last] = tau
        with np.errstate(over="ignore", under="ignore"):
            out["trans", from_last] = np.exp(-tau)
        start = cases.boundary_start(kind, v.nu, v.boundary_t, v.boundary_e)
        rad, _ = cases.sweep_radiance(kind, v.nu, v.beta, v.thickness, v.temperature, n,
                                      from_last, start)
        out["rad", from_last] = rad
        out["bt", from_last] = cases.brightness(kind, v.nu, cases.flushed(rad))
        lengths, weight = v.lengths(3)
        down = cases.sweep_flux(kind, v.nu, v.beta, lengths, weight, v.temperature, n, from_last)
        start, _ = cases.surface_start(kind, v.nu, v.surface_t, v.surface_e, down.total,
                                       down.total_mag)
        up = cases.sweep_flux(kind, v.nu, v.beta, lengths, weight, v.temperature, n,
                              not from_last, start)
        out["down", from_last], out["up", from_last] = down.flux, up.flux
        out["reflection", from_last] = down.total
    return v, out


def test_extreme_values_have_one_pattern_in_float64_and_long_double():
    v, loop = value_sweeps(F64)
    _, reference = value_sweeps(LD)
    tiny = np.finfo(F64).tiny
    for key, values in loop.items():
        assert cases.same_pattern(values, reference[key]), key
        assert not np.any(np.isnan(values)) and not np.any(np.isinf(values)), key
        # nothing lands among the subnormals, where float64 and long double part
        assert not np.any((values != 0.) & (np.abs(values) < tiny)), key
        wide = np.abs(reference[key])
        assert not np.any((wide > LD("1e-330")) & (wide < tiny)), key
    # and the table holds what it claims
    n, group = v.levels_per_path, v.group
    for from_last in (False, True):
        last = cases._flat(n, 0 if from_last else n - 1)
        assert np.all(loop["tau", from_last][:, group == 0] == 0.)
        assert np.all(loop["trans", from_last][:, group == 0] == 1.)
        assert np.all(loop["trans", from_last][last][:, group == 1] == 0.)
        start = cases.boundary_start(F64, v.nu, v.boundary_t, v.boundary_e)
        rad = loop["rad", from_last]
        assert np.array_equal(rad[:, group == 0],
                              np.repeat(start, n, axis=0)[:, group == 0])
        saturated = cases.planck(F64, v.nu, v.temperature[last, None])[:, group == 1]
        assert np.allclose(rad[last][:, group == 1], saturated, rtol=1e-15, atol=0.)
        assert np.all(rad[:, 0] == 0.) and np.all(loop["bt", from_last][:, 0] == 0.)
        assert np.all(loop["down", from_last][:, 0] == 0.)
        assert np.any(rad[:, group == 2] < 0.) and np.any(rad[:, group == 2] > 0.)
    high = v.nu >= 2000.
    assert np.all(cases.planck(F64, v.nu[high], 1.) == 0.)
    assert np.all(cases.planck(F64, v.nu[high], 320.) > 0.)
    cold = cases.boundary_start(F64, v.nu, v.boundary_t, v.boundary_e)[2]
    assert np.any(cold[high] == 0.) and np.any((cold[high] > 0.) & (cold[high] < 1e-200))
