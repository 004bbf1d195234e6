"""What tests/test_linear_source_host.py (CPU), tests/test_gpu_linear_source_shapes.py and
tests/test_gpu_linear_source.py (GPU) share: the linear-in-tau update of include/lbl_amd.h
(lbl_path_radiance_source, lbl_path_flux_source) in numpy.  In numpy.longdouble it is the
reference: the weight w = 1 - a/x comes from a 24-term series below |x| = 0.5 and from 1 - a/x
above, nothing of the form under test.  In float64 `device_weight` is the form the header states,
term by term.  Each sweep returns its companion magnitude, the sum over levels of
|I_in|*t + (|B_in| + |B_out|)*|a|, against which the 1e-12 bound of the suite is taken."""
import math

import numpy as np

from tests import sweep_cases as cases

LD = np.longdouble
PATHS = cases.PATHS
SERIES_BELOW = 1./16.       # kLinearSeriesBelow of csrc/radiance.h
SERIES_TERMS = 8


def device_weight(x):
    """w as the kernels form it, in float64, every product and sum rounded as written."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        a = -np.expm1(-x)
        series = x*(1./2. - x*(1./6. - x*(1./24. - x*(1./120. - x*(1./720. - x*(1./5040. - x*(
            1./40320. - x*(1./362880.))))))))
        return np.where(np.abs(x) < SERIES_BELOW, series, 1. - a/x)


def naive_weight(x):
    """1 - a/x in float64 everywhere: what the kernels must not do."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        return 1. - (-np.expm1(-x))/x


def weight(kind, x):
    """The reference w = 1 - a/x in the float type `kind`: sum_{n>=1} (-1)^(n+1) x^n/(n+1)! in 24
    terms (Horner) below |x| = 0.5, where the 25th is below 2^-24/26! of the first, and 1 - a/x
    above, where a/x is at most 0.79 or at least 1.29 and the difference loses under a bit."""
    x = np.asarray(x, dtype=kind)
    one = kind(1.)
    series = np.zeros(x.shape, dtype=kind)
    for n in range(24, 0, -1):
        series = one/kind(math.factorial(n + 1)) - x*series
    series = x*series
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        direct = one - (-np.expm1(-x))/x
    return np.where(np.abs(x) < kind(0.5), series, direct)


def update(kind, rad, mag, x, b_in, b_out):
    """One level: (I*t + (B_in*u_in + B_out*w), |I|*t + (|B_in| + |B_out|)*|a|) in `kind`; with
    float64 the weight is the device's form."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t, a = np.exp(-x), -np.expm1(-x)
        w = device_weight(x) if kind is np.float64 else weight(kind, x)
        rad = rad*t + (b_in*(a - w) + b_out*w)
        mag = mag*t + (np.abs(b_in) + np.abs(b_out))*np.abs(a)
    return rad, mag


def edge_table(interfaces):
    """[paths, L + 1] interface temperatures as the entries' [levels][2] table."""
    interfaces = np.asarray(interfaces, dtype=np.float64)
    edges = np.stack([interfaces[:, :-1], interfaces[:, 1:]], axis=-1)
    return np.ascontiguousarray(edges.reshape(-1, 2))


def interfaces_for(problem, seed):
    """Random interface temperatures [PATHS, L + 1] for a sweep_cases.Problem."""
    rng = np.random.default_rng(seed)
    return rng.uniform(150., 320., size=(PATHS, problem.levels_per_path + 1))


def _edge_planck(kind, nu, edges, rows, side):
    return cases.planck(kind, nu, edges[rows, side].astype(kind)[:, None])


def sweep_radiance(kind, nu, beta, lengths, edges, levels_per_path, from_last=False, start=None):
    """The linear update for all PATHS paths from `start` [PATHS, columns] (None: 0): (I,
    magnitude) after every level, [levels, columns].  The level's entry interface is [.][0]
    upward and [.][1] from the last level down."""
    beta, lengths = beta.astype(kind), lengths.astype(kind)
    shape = (PATHS, beta.shape[1])
    rad = np.zeros(shape, dtype=kind) if start is None else np.array(start, dtype=kind)
    mag = np.abs(rad)
    out, mags = np.zeros(beta.shape, dtype=kind), np.zeros(beta.shape, dtype=kind)
    enter, leave = (1, 0) if from_last else (0, 1)
    for step in cases._sweep_order(levels_per_path, from_last):
        rows = cases._flat(levels_per_path, step)
        x = lengths[rows, None]*beta[rows]
        rad, mag = update(kind, rad, mag, x, _edge_planck(kind, nu, edges, rows, enter),
                          _edge_planck(kind, nu, edges, rows, leave))
        out[rows], mags[rows] = rad, mag
    return out, mags


def sweep_flux(kind, nu, beta, lengths, weight_, edges, levels_per_path, from_last=False,
               start=None, start_mag=None):
    """sweep_cases.sweep_flux with the linear update: a FluxSweep."""
    beta, lengths = beta.astype(kind), lengths.astype(kind)
    weight_ = weight_.astype(kind)
    angles = weight_.size
    shape = (PATHS, angles, beta.shape[1])
    rad, mag = np.zeros(shape, dtype=kind), np.zeros(shape, dtype=kind)
    if start is not None:
        rad = rad + np.asarray(start, dtype=kind)[:, None, :]
        mag = mag + np.asarray(np.abs(start) if start_mag is None else start_mag,
                               dtype=kind)[:, None, :]
    levels = beta.shape[0]
    flux, flux_mag = (np.zeros(beta.shape, dtype=kind) for _ in range(2))
    rads, rad_mags = (np.zeros((levels,) + shape[1:], dtype=kind) for _ in range(2))
    pi = kind(cases.FLUX_PI)
    enter, leave = (1, 0) if from_last else (0, 1)
    for step in cases._sweep_order(levels_per_path, from_last):
        rows = cases._flat(levels_per_path, step)
        x = lengths[rows][:, :, None]*beta[rows][:, None, :]
        rad, mag = update(kind, rad, mag, x,
                          _edge_planck(kind, nu, edges, rows, enter)[:, None, :],
                          _edge_planck(kind, nu, edges, rows, leave)[:, None, :])
        rads[rows], rad_mags[rows] = rad, mag
        flux[rows] = pi*cases.flux_sum(weight_, rad)
        flux_mag[rows] = pi*cases.flux_sum(weight_, mag)
    return cases.FluxSweep(flux, flux_mag, rads, rad_mags, cases.flux_sum(weight_, rad),
                           cases.flux_sum(weight_, mag))


def weight_samples(count=500000, seed=5):
    """The sample ranges of the weight check: x log-uniform from 1e-12 to 1e3, and negative x
    log-uniform from -1e-12 down to -3, with the thresholds of both forms and their neighbours."""
    rng = np.random.default_rng(seed)
    positive = 10.**rng.uniform(-12., 3., size=(4*count)//5)
    negative = -10.**rng.uniform(-12., math.log10(3.), size=count//5)
    edge = np.array([SERIES_BELOW, 0.5, 1e-12, 1e3, 3., 50., 700.])
    near = np.concatenate([edge, np.nextafter(edge, 0.), np.nextafter(edge, np.inf)])
    near = np.concatenate([near, -near[np.abs(near) <= 3.]])
    return np.concatenate([positive, negative, near])
