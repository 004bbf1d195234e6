"""What tests/test_surface_host.py (CPU), tests/test_gpu_surface_shapes.py and
tests/test_gpu_surface.py (GPU) share: the surface of compute_radiance as include/lbl_amd.h states
it (lbl_surface_emissivity, lbl_path_radiance_surface) in numpy -- the interpolation of an
emissivity table onto a grid and the two-pass recurrence (down pass, start value, up pass) on the
sweeps of tests/sweep_cases.py and tests/linear_source_cases.py, in any float type: float64 "as
written", numpy.longdouble as the reference -- and a recording engine for the queue of a call.

Magnitudes: the sweeps' own recurrence over absolute values, started from |E|*B + |1 - E|*|D|
with |D| the magnitude of the down pass; the suite's 1e-12 bound is taken against it."""
import contextlib

import numpy as np

from tests import absorption_recorder as recorder
from tests import linear_source_cases as linear
from tests import sweep_cases as cases

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
MAX_KNOTS = 1024            # kSurfaceMaxKnots of csrc/surface.h
DOWNWELLING = "boundary_downwelling_radiance"


# ---------------------------------------------------------------------------------------------
# The interpolation.
def interval(knots, nu):
    """The number of knots <= nu, less one, and -1 for nu <= k_0 (on the knot too) and NaN: a
    loop over the knots, nothing of numpy's searches."""
    knots, nu = np.asarray(knots), np.asarray(nu)
    count = np.zeros(nu.shape, dtype=np.int64)
    for knot in knots:
        count += knot <= nu
    return np.where(nu > knots[0], count - 1, -1)


def emissivity(kind, knots, values, nu):
    """E [..., columns] of the tables `values` [..., M] at the knots [M] on the points nu, every
    operation in `kind` and rounded as written:
    E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j)) for k_j <= nu < k_{j+1}, e_0 for
    nu <= k_0, e_{M-1} for nu >= k_{M-1}."""
    k = np.asarray(knots, dtype=F64).astype(kind)
    e = np.asarray(values, dtype=F64).astype(kind)
    x = np.asarray(nu, dtype=F64).astype(kind)
    last = k.size - 1
    j = interval(k, x)
    inner = np.clip(j, 0, last - 1)
    with np.errstate(over="ignore", invalid="ignore"):
        slope = (e[..., inner + 1] - e[..., inner])/(k[inner + 1] - k[inner])
        inside = e[..., inner] + (x - k[inner])*slope
    return np.where(j < 0, e[..., :1], np.where(j >= last, e[..., last:], inside))


# The written formula in float64 against the exact line through the two knots, for e in [0, 1]:
# with h = k_{j+1} - k_j and d = e_{j+1} - e_j, the differences nu - k_j, h and d and the quotient
# and the product round once each, to at most (1 + u)^4 - 1 relative of a product that is at most
# |d| <= 1 (since 0 <= nu - k_j < h), and the final sum rounds a value of at most 1 + 4u once more:
# 4u + u = 5u <= 5.6e-16 absolute with u = 2^-53; the bound below leaves the second-order terms
# and the long-double reference's own 2^-64 roundings room.
INTERPOLATION_BOUND = 6e-16


def knot_samples(knots):
    """Points that hit every knot, lie 1 ulp on either side of it, between knots, and below and
    above all of them."""
    knots = np.asarray(knots, dtype=F64)
    middle = (knots[:-1] + knots[1:])/2.
    outside = np.array([knots[0] - 1., knots[0] - 1e-9, -knots[-1], knots[-1] + 1e-9,
                        knots[-1]*2. + 1., 0.])
    return np.concatenate([knots, np.nextafter(knots, -np.inf), np.nextafter(knots, np.inf),
                           middle, outside])


# ---------------------------------------------------------------------------------------------
# The two passes.
def surface_start(kind, nu, boundary_t, e, down=None, down_mag=None):
    """(I, magnitude) [PATHS, columns] a path starts from: E*B(nu, T_b) + (1. - E)*D -- E*B alone
    without D -- and |E|*B + |1 - E|*|D|; 0 where T_b is 0.  e: [PATHS] (scalars) or
    [PATHS, columns]."""
    t = np.asarray(boundary_t, dtype=kind)[:, None]
    e = np.asarray(e, dtype=F64).astype(kind)
    if e.ndim == 1:
        e = e[:, None]
    safe = np.where(t > 0., t, kind(1.))
    emitted = e*cases.planck(kind, nu, safe)
    start, mag = emitted, np.abs(emitted)
    if down is not None:
        one = kind(1.)
        start = emitted + (one - e)*np.asarray(down, dtype=kind)
        mag = np.abs(emitted) + np.abs(one - e)*np.asarray(down_mag, dtype=kind)
    return np.where(t > 0., start, kind(0.)), np.where(t > 0., mag, kind(0.))


def _sweep(kind, problem, lengths, from_last, start, edges):
    if edges is None:
        return cases.sweep_radiance(kind, problem.nu, problem.beta, lengths, problem.temperature,
                                    problem.levels_per_path, from_last, start)
    return linear.sweep_radiance(kind, problem.nu, problem.beta, lengths, edges,
                                 problem.levels_per_path, from_last, start)


def final_rows(levels_per_path, from_last):
    return cases._flat(levels_per_path, 0 if from_last else levels_per_path - 1)


def restart(kind, problem, lengths, from_last, start, start_mag, edges):
    """A sweep from (start, start_mag).  The sweeps of sweep_cases start their magnitude from
    |start|; a reflecting start is formed from more than that, so the magnitude is the same
    sweep started from start_mag (>= 0), whose own magnitude it is."""
    rad, _ = _sweep(kind, problem, lengths, from_last, start, edges)
    _, mag = _sweep(kind, problem, lengths, from_last, start_mag, edges)
    return rad, mag


def two_pass(kind, problem, from_last, e, reflection_lengths=None, edges=None):
    """{"down": (D, |D|) [PATHS, columns] or None, "start": (I, magnitude), "up": (I, magnitude)
    [levels, columns]} of a call in `direction`: the down pass against it with
    reflection_lengths from 0, then the up pass from the start value.  e: [PATHS] or
    [PATHS, columns]."""
    down = None
    if reflection_lengths is not None:
        rad, mag = _sweep(kind, problem, np.asarray(reflection_lengths), not from_last, None,
                          edges)
        rows = final_rows(problem.levels_per_path, not from_last)
        down = (rad[rows], mag[rows])
    start, start_mag = surface_start(kind, problem.nu, problem.boundary_t, e,
                                     *(down if down is not None else (None, None)))
    up = restart(kind, problem, problem.thickness, from_last, start, start_mag, edges)
    return {"down": down, "start": (start, start_mag), "up": up}


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class SurfaceRecorder(recorder.RecordingEngine):
    """tests/absorption_recorder.py's engine with the radiance calls."""
    def path_radiance(self, beta, columns, grid, n_paths, levels_per_path, level_begin, lengths,
                      temperature, carry, **keywords):
        described = {name: (np.asarray(value) if isinstance(value, (list, tuple, np.ndarray))
                            else value) for name, value in sorted(keywords.items())}
        self.record("path_radiance", beta=beta, columns=columns, grid=grid, n_paths=n_paths,
                    levels_per_path=levels_per_path, level_begin=level_begin,
                    lengths=np.asarray(lengths), temperature=np.asarray(temperature),
                    carry=carry, **described)

    def surface_emissivity(self, grid, rows, knot_wavenumber, knot_emissivity, path_begin=0,
                           asynchronous=False):
        self.record("surface_emissivity", grid=grid, rows=rows,
                    knot_wavenumber=np.asarray(knot_wavenumber),
                    knot_emissivity=np.asarray(knot_emissivity), path_begin=path_begin,
                    asynchronous=asynchronous)


class Untouchable(object):
    """An engine that fails on any use."""
    def __getattr__(self, name):
        raise AssertionError("the engine was reached: %s" % name)


SHAPE = (2, 3)              # 2 paths of 3 levels on absorption_recorder.GRID (rows of 164)
ROW_BYTES = 164*8


@contextlib.contextmanager
def recorded(directory, gas_set="lighter second"):
    """(Spectroscopy of SHAPE on a SurfaceRecorder, the engine), installed as every back end's
    engine while the block runs."""
    before = recorder.RecordingEngine
    recorder.RecordingEngine = SurfaceRecorder
    try:
        spec, engine = recorder.spectroscopy(gas_set, int(np.prod(SHAPE)), directory, shape=SHAPE)
    finally:
        recorder.RecordingEngine = before
    for name, value in recorder.DEFAULTS.items():
        setattr(spec, name, value)
    with recorder.installed(engine):
        yield spec, engine


def interfaces():
    return np.linspace(205., 295., SHAPE[0]*(SHAPE[1] + 1)).reshape(SHAPE[0], SHAPE[1] + 1)


def default_calls():
    """{name: (device_output_limit in rows, keywords)}: calls of compute_radiance that use
    nothing of the surface -- what tests/golden/radiance_default_queue.json records."""
    lengths = np.linspace(50., 300., 6).reshape(SHAPE)
    return {
        "plain": (None, dict(path_length=lengths, boundary_temperature=288.,
                             boundary_emissivity=0.9)),
        "toward first, both quantities": (None, dict(
            path_length=lengths, boundary_temperature=[288., 275.],
            boundary_emissivity=[0.9, 1.], direction="toward_first",
            quantities=("radiance", "brightness_temperature"))),
        "bands, cumulative": (None, dict(path_length=lengths, boundary_temperature=288.,
                                         band_edges=[20., 30., 45., 60.], cumulative=True)),
        "runs of two levels, linear": (2, dict(
            path_length=lengths, boundary_temperature=288., boundary_emissivity=0.5,
            source="linear_in_tau", interface_temperature=interfaces())),
        "no boundary, pedestal kept": (4, dict(path_length=lengths, remove_pedestal=False,
                                               direction="toward_first")),
    }


def queue_of(spec, engine, limit_rows, keywords):
    """The log of spec.compute_radiance(**keywords) with device_output_limit = limit_rows rows."""
    spec.device_output_limit = (8 << 30) if limit_rows is None else limit_rows*ROW_BYTES
    engine.begin()
    spec.compute_radiance(**keywords)
    return list(engine.log)


def default_queues(directory):
    with recorded(directory) as (spec, engine):
        return {name: queue_of(spec, engine, limit, keywords)
                for name, (limit, keywords) in default_calls().items()}
