"""What the Jacobian tests share (tests/test_jacobian_host.py on the CPU, tests/test_gpu_jacobian*.py
on the GPU): lbl_path_jacobian's formulas of include/lbl_amd.h in numpy, in any float type (float64
"in the stated order", numpy.longdouble as the reference), with the magnitude each result is formed
from, and the inputs the CPU test differentiates numerically."""
import numpy as np

from pylbl_amd.spectroscopy import PLANCK_C1
from tests import sweep_cases as cases

LD = np.longdouble
PER_LEVEL = ("optical_depth_jacobian", "log_optical_depth_jacobian", "temperature_jacobian")
PER_PATH = ("radiance", "boundary_temperature_jacobian", "boundary_emissivity_jacobian")
QUANTITIES = PER_LEVEL + PER_PATH
# Engine.path_jacobian's outputs in the order of their flags' bits (radiance's is the lowest).
OUTPUTS = ("radiance",) + PER_LEVEL + PER_PATH[1:]

# Levels per path below, at, above and beyond twice the rows in flight of the kernel's loop 1
# (kPathAhead = 8) and loop 2 (kJacobianAhead).
JACOBIAN_AHEAD = 4
DEPTHS = (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 15, 16, 17, 19, 33)


def planck_dt(kind, nu, temperature):
    """dB(nu, T) = (B*(u/T))*(1. + B/(((C1*nu)*nu)*nu)), u = (C2*nu)/T; 0 for nu <= 0."""
    nu, temperature = np.asarray(nu, dtype=kind), np.asarray(temperature, dtype=kind)
    b = cases.planck(kind, nu, temperature)
    c1 = kind(PLANCK_C1)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore", under="ignore"):
        u = (kind(cases.PLANCK_C2)*nu)/temperature
        d = (b*(u/temperature))*(kind(1.) + b/(((c1*nu)*nu)*nu))
    return np.where(nu > 0., d, kind(0.))


def jacobian(kind, nu, beta, lengths, temperature, levels_per_path, from_last=False,
             boundary_t=None, boundary_e=None):
    """(values, magnitudes): {quantity: [levels, columns] per level, [paths, columns] per path} for
    beta [levels, columns] of paths of levels_per_path consecutive levels, lengths and temperature
    [levels], boundary_t (None or 0: no boundary) and boundary_e [paths] -- every product and sum
    rounded as the header writes it.  The magnitudes are what the project's 1e-12 applies to:
    (|B_k| + M_k)*trail_k for dI/dx with M_k the magnitude of I_k (the forward recurrence over
    absolute values, |I_k| itself for beta >= 0), |x_k| times that for dI/dln x, M_{L-1} for the
    radiance, and the value itself for the temperature and boundary Jacobians."""
    n = levels_per_path
    levels, columns = beta.shape
    paths = levels//n
    assert paths*n == levels
    beta = np.asarray(beta).astype(kind).reshape(paths, n, columns)
    s = np.asarray(lengths).astype(kind).reshape(paths, n, 1)
    t = np.asarray(temperature).astype(kind).reshape(paths, n, 1)
    nu = np.asarray(nu).astype(kind)
    tb = np.zeros(paths, dtype=kind) if boundary_t is None else np.asarray(boundary_t).astype(kind)
    eb = np.ones(paths, dtype=kind) if boundary_e is None else np.asarray(boundary_e).astype(kind)
    has = (tb > 0.)[:, None]
    safe = np.where(tb > 0., tb, kind(1.))[:, None]
    order = list(range(n - 1, -1, -1) if from_last else range(n))
    zero = kind(0.)

    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        # Trailing optical depth, from the observer backwards.
        tau = np.zeros((paths, columns), dtype=kind)
        trail = np.zeros(beta.shape, dtype=kind)
        for level in reversed(order):
            trail[:, level] = np.exp(-tau)
            tau = tau + s[:, level]*beta[:, level]
        trail_b = np.exp(-tau)
        source_b = np.where(has, cases.planck(kind, nu, safe), zero)
        values = {
            "boundary_temperature_jacobian":
                np.where(has, (eb[:, None]*planck_dt(kind, nu, safe))*trail_b, zero),
            "boundary_emissivity_jacobian": source_b*trail_b}
        magnitudes = {q: np.abs(v) for q, v in values.items()}
        # Forward.
        rad = np.where(has, eb[:, None]*source_b, zero)
        mag = np.abs(rad)
        for q in PER_LEVEL:
            values[q] = np.zeros(beta.shape, dtype=kind)
            magnitudes[q] = np.zeros(beta.shape, dtype=kind)
        for level in order:
            x = s[:, level]*beta[:, level]
            source = cases.planck(kind, nu, t[:, level])
            emitted = -np.expm1(-x)
            rad = rad*np.exp(-x) + source*emitted
            mag = mag*np.exp(-x) + np.abs(source*emitted)
            dx = (source - rad)*trail[:, level]
            formed = (np.abs(source) + mag)*trail[:, level]
            values["optical_depth_jacobian"][:, level] = dx
            magnitudes["optical_depth_jacobian"][:, level] = formed
            values["log_optical_depth_jacobian"][:, level] = x*dx
            magnitudes["log_optical_depth_jacobian"][:, level] = np.abs(x)*formed
            dt = (emitted*planck_dt(kind, nu, t[:, level]))*trail[:, level]
            values["temperature_jacobian"][:, level] = dt
            magnitudes["temperature_jacobian"][:, level] = np.abs(dt)
        values["radiance"], magnitudes["radiance"] = rad, mag
    for store in (values, magnitudes):
        for q in PER_LEVEL:
            store[q] = store[q].reshape(levels, columns)
    return values, magnitudes


class SmoothProblem(object):
    """The inputs the formulas are differentiated on: cases.PATHS paths of 40 levels on 4000
    points, beta 1e-9 .. 1e-2 m-1, s 50 .. 2000 m, T 190 .. 310 K, T_b 295 K, eps 0.97."""
    def __init__(self, levels_per_path=40, columns=4000, seed=5):
        rng = np.random.default_rng(seed)
        levels = cases.PATHS*levels_per_path
        self.levels_per_path, self.columns, self.levels = levels_per_path, columns, levels
        self.nu = np.linspace(50., 2800., columns)
        self.beta = 10.**rng.uniform(-9., -2., size=(levels, columns))
        self.lengths = rng.uniform(50., 2000., size=levels)
        self.temperature = rng.uniform(190., 310., size=levels)
        self.boundary_t = np.full(cases.PATHS, 295.)
        self.boundary_e = np.full(cases.PATHS, 0.97)

    def radiance(self, lengths=None, temperature=None, boundary_t=None, boundary_e=None,
                 from_last=False):
        """cases.sweep_radiance's final radiance in long double: [PATHS, columns]."""
        n = self.levels_per_path
        start = cases.boundary_start(
            LD, self.nu, self.boundary_t if boundary_t is None else boundary_t,
            self.boundary_e if boundary_e is None else boundary_e)
        rad, _ = cases.sweep_radiance(
            LD, self.nu, self.beta, np.asarray(self.lengths if lengths is None else lengths, LD),
            np.asarray(self.temperature if temperature is None else temperature, LD), n,
            from_last, start)
        return rad[cases._flat(n, 0 if from_last else n - 1)]
