"""What tests/test_two_stream_host.py (CPU), tests/test_gpu_two_stream_shapes.py and
tests/test_gpu_two_stream.py (GPU) share: the definition of Spectroscopy.compute_solar_flux in
numpy -- the layer of csrc/twostream.h and the adding recurrences, for any float type: float64
"as written", numpy.longdouble as the reference -- the Rayleigh fit, a stand-in engine with the
two calls, and the case tables.  Columns, layouts and bands are tests/sweep_cases.py's.

The layer's inputs (t, w, gp and the branch decisions: identity, conservative, resonance guard
and its side) are formed in float64, as the host and the kernel form them; a reference in another
float type continues from those.

E_CPU is the worst |float64 mirror - long-double mirror|/F0 over every case table of this file,
as tests/test_two_stream_host.py measures it; the GPU tests hold every flux to
(4*E_CPU + 1e-13)*F0 of the long-double mirror."""
import contextlib

import numpy as np

from pylbl_amd import paths
from tests import solar_cases as solar
from tests import surface_cases as surface
from tests import sweep_cases as cases

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
CONSERVATIVE = 1e-10        # kTwoStreamConservative
RESONANCE = 1e-4            # kTwoStreamResonance
UP_AHEAD, DOWN_AHEAD = 8, 1  # kTwoStreamUpAhead, kTwoStreamDownAhead
QUANTITIES = ("up", "down", "direct", "diffuse")
# The worst error of the float64 mirror over the case tables, relative to F0 (see above).
E_CPU = 1.7e-11
E_CPU_CAP = 1e-10
FLUX_FLOOR = 1e-13

IDENTITY, CONSERVATIVE_BRANCH, GENERAL, GUARDED = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------------
# The layer.
def layer_inputs(table, mu0, beta, sigma):
    """What the kernel forms in float64 before the branches, each rounded as written: a dict of
    t, w, gp, k2, the branch code per element and the guard's side.  table [..., 5] (s_l, c_l,
    tau_c, w_c, h_c), mu0 broadcastable to the elements, beta and sigma float64."""
    table = np.asarray(table, dtype=F64)
    s, c, tau_c, w_c, h_c = (table[..., i] for i in range(5))
    beta, sigma, mu0 = (np.asarray(x, dtype=F64) for x in (beta, sigma, mu0))
    with np.errstate(all="ignore"):
        tau_a = s*beta
        tau_r = c*sigma
        tau = (tau_a + tau_r) + tau_c
        tau_s = tau_r + w_c
        omega = tau_s/tau
        g = np.where(tau_s == 0., 0., h_c/np.where(tau_s == 0., 1., tau_s))
        f = g*g
        sc = 1. - omega*f
        t = sc*tau
        w = ((1. - f)*omega)/sc
        gp = g/(1. + g)
        g2 = (3.*(w*(1. - gp)))/4.
        dif = 2.*(1. - w)
        g1 = g2 + dif
        su = g1 + g2
        k2 = dif*su
        x = np.sqrt(np.where(k2 > 0., k2, 0.))*mu0
        conservative = k2*(1. + t*t) <= CONSERVATIVE
        guarded = np.abs(1. - x) < RESONANCE
    branch = np.where(tau == 0., IDENTITY,
                      np.where(conservative, CONSERVATIVE_BRANCH,
                               np.where(guarded, GUARDED, GENERAL)))
    shape = branch.shape
    return {"t": np.broadcast_to(t, shape), "w": np.broadcast_to(w, shape),
            "gp": np.broadcast_to(gp, shape), "k2": np.broadcast_to(k2, shape),
            "x": np.broadcast_to(x, shape), "branch": branch,
            "above": np.broadcast_to(x >= 1., shape), "tau": np.broadcast_to(tau, shape),
            "mu0": np.broadcast_to(mu0, shape)}


def layer(kind, inputs):
    """(Rdif, Tdif, Rdir, Tdp, D) in `kind` from layer_inputs' float64 t, w, gp and branches, every
    operation rounded as written."""
    one, two, three, four = kind(1.), kind(2.), kind(3.), kind(4.)
    t, w, gp, mu0 = (inputs[name].astype(kind) for name in ("t", "w", "gp", "mu0"))
    branch = inputs["branch"]
    with np.errstate(all="ignore"):
        g2 = (three*(w*(one - gp)))/four
        dif = two*(one - w)
        g1 = g2 + dif
        su = g1 + g2
        g3 = (two - three*(mu0*gp))/four
        g4 = one - g3
        k2 = dif*su
        d = np.exp(-t/mu0)
        # Conservative.
        x = g1*t
        c_rdif = x/(one + x)
        c_tdif = one/(one + x)
        c_rdir = (x + (g3 - g1*mu0)*(-np.expm1(-t/mu0)))/(one + x)
        c_tdp = (one - c_rdir) - d
        # General.
        k = np.sqrt(np.where(k2 > 0., k2, one))
        side = np.where(inputs["above"], one + kind(RESONANCE), one - kind(RESONANCE))
        m = np.where(branch == GUARDED, side/k, mu0)
        x = k*m
        dm = np.where(branch == GUARDED, np.exp(-t/m), d)
        e = np.exp(-(k*t))
        e2 = e*e
        o1 = -np.expm1(-(two*(k*t)))
        den = k*(one + e2) + g1*o1
        q = ((one - x)*(one + x))*den
        rdif = (g2*o1)/den
        tdif = (two*(k*e))/den
        a1 = g1*g4 + g2*g3
        a2 = g1*g3 + g2*g4
        rdir = w*((one - x)*(a2 + k*g3) - ((one + x)*(a2 - k*g3))*e2 -
                  (two*(k*(g3 - a2*m)))*(e*dm))/q
        ttot = dm*(one - w*((one + x)*(a1 + k*g4) - ((one - x)*(a1 - k*g4))*e2)/q) + \
            w*((two*(k*(g4 + a1*m)))*e)/q
        tdp = ttot - dm

    def pick(identity, conservative, general):
        return np.where(branch == IDENTITY, kind(identity),
                        np.where(branch == CONSERVATIVE_BRANCH, conservative, general))
    return (pick(0., c_rdif, rdif), pick(1., c_tdif, tdif), pick(0., c_rdir, rdir),
            pick(0., c_tdp, tdp), pick(1., d, d))


# ---------------------------------------------------------------------------------------------
# Adding.
def adding(kind, layers, albedo, f0):
    """The adding recurrences over layers[i] = (Rdif, Tdif, Rdir, Tdp, D) of L levels in the
    Sun's order (each [L, ...]), a Lambertian albedo [...] and F0 [...]: {"up", "down", "direct",
    "diffuse"} at the L + 1 interfaces [L + 1, ...] (interface 0 faces space), and "rup", "rupd"."""
    rdif, tdif, rdir, tdp, d = layers
    levels = rdif.shape[0]
    one = kind(1.)
    albedo = np.broadcast_to(np.asarray(albedo, dtype=F64).astype(kind), rdif.shape[1:])
    f0 = np.broadcast_to(np.asarray(f0, dtype=F64).astype(kind), rdif.shape[1:])
    rup = np.zeros((levels + 1,) + rdif.shape[1:], dtype=kind)
    rupd = np.zeros_like(rup)
    rup[levels] = rupd[levels] = albedo
    with np.errstate(all="ignore"):
        for i in range(levels - 1, -1, -1):
            m1 = one/(one - rdif[i]*rupd[i + 1])
            rup[i] = rdir[i] + tdif[i]*((tdp[i]*rupd[i + 1] + d[i]*rup[i + 1])*m1)
            rupd[i] = rdif[i] + tdif[i]*((tdif[i]*rupd[i + 1])*m1)
        out = {name: np.zeros_like(rup) for name in QUANTITIES}
        tb = np.ones(rdif.shape[1:], dtype=kind)
        td = np.zeros_like(tb)
        rd = np.zeros_like(tb)
        for i in range(levels + 1):
            m2 = one/(one - rd*rupd[i])
            out["direct"][i] = f0*tb
            out["diffuse"][i] = f0*((td + (tb*rup[i])*rd)*m2)
            out["up"][i] = f0*((tb*rup[i] + td*rupd[i])*m2)
            out["down"][i] = out["direct"][i] + out["diffuse"][i]
            if i == levels:
                break
            m3 = one/(one - rd*rdif[i])
            td = tb*tdp[i] + tdif[i]*((td + (tb*rd)*rdir[i])*m3)
            rd = rdif[i] + tdif[i]*((tdif[i]*rd)*m3)
            tb = tb*d[i]
    out["rup"], out["rupd"] = rup, rupd
    return out


def column(kind, table, mu0, beta, sigma, albedo, f0):
    """One or more columns in the Sun's order: table [L, 5], beta [L, ...], sigma, albedo and f0
    [...]; adding()'s result."""
    table = np.asarray(table, dtype=F64)
    beta = np.asarray(beta, dtype=F64)
    lead = (slice(None),) + (None,)*(beta.ndim - 1)
    inputs = layer_inputs(table[lead], mu0, beta, sigma)
    return adding(kind, layer(kind, inputs), albedo, f0)


# ---------------------------------------------------------------------------------------------
# A problem of PATHS paths in flat storage, as lbl_path_two_stream takes it.
class Inputs(object):
    """beta [levels, columns], table [levels, 5], mu0 [PATHS], solar and sigma [columns], albedo
    [PATHS] or [PATHS, columns]."""
    def __init__(self, name, beta, table, mu0, solar_row, sigma, albedo):
        self.name = name
        self.beta = np.ascontiguousarray(beta, dtype=F64)
        self.table = np.ascontiguousarray(table, dtype=F64)
        self.mu0 = np.asarray(mu0, dtype=F64)
        self.solar, self.sigma = np.asarray(solar_row, F64), np.asarray(sigma, F64)
        self.albedo = np.asarray(albedo, dtype=F64)
        self.levels, self.columns = self.beta.shape
        self.levels_per_path = self.levels//PATHS
        assert self.table.shape == (self.levels, 5) and self.levels % PATHS == 0

    def f0(self):
        return self.mu0[:, None]*self.solar[None, :]

    def sun_order(self, from_last):
        """[PATHS, L] flat levels, each path's in the Sun's order."""
        n = self.levels_per_path
        flat = np.arange(self.levels).reshape(PATHS, n)
        return flat[:, ::-1] if from_last else flat

    def layer_inputs(self, from_last):
        """layer_inputs of every element: arrays [L, PATHS, columns] in the Sun's order."""
        order = self.sun_order(from_last).T                      # [L, PATHS]
        return layer_inputs(self.table[order][:, :, None, :], self.mu0[None, :, None],
                            self.beta[order], self.sigma[None, None, :])


def mirror(kind, inputs, from_last):
    """{quantity: [levels, columns] at the interface below each flat level, "top_" + quantity:
    [PATHS, columns] at interface 0} in `kind`; "f0" [PATHS, columns] in float64."""
    order = inputs.sun_order(from_last).T
    albedo = inputs.albedo[:, None] if inputs.albedo.ndim == 1 else inputs.albedo
    f0 = inputs.f0()
    result = adding(kind, layer(kind, inputs.layer_inputs(from_last)), albedo, f0)
    out = {"f0": f0}
    for q in QUANTITIES:
        below = np.zeros((inputs.levels, inputs.columns), dtype=kind)
        below[order] = result[q][1:]
        out[q], out["top_" + q] = below, result[q][0]
    return out


def worst_error(inputs, from_last):
    """The worst |float64 mirror - long-double mirror|/F0 of the four fluxes at every interface
    (columns with F0 = 0 must agree exactly), and whether everything is finite."""
    low, high = mirror(F64, inputs, from_last), mirror(LD, inputs, from_last)
    f0 = low["f0"]
    worst, finite = 0., True
    per_level = np.repeat(f0, inputs.levels_per_path, axis=0)
    for q in QUANTITIES:
        for name, scale in ((q, per_level), ("top_" + q, f0)):
            finite = finite and bool(np.all(np.isfinite(low[name])))
            error = np.abs(low[name].astype(LD) - high[name])
            dark = scale == 0.
            assert np.all(error[dark] == 0.)
            if np.any(~dark):
                worst = max(worst, float(np.max(error[~dark]/scale[~dark])))
    return worst, finite


# ---------------------------------------------------------------------------------------------
# The Rayleigh fit.
def rayleigh(kind, nu):
    """sigma(nu) [m2] as lbl_rayleigh_row forms it, in `kind` from the float64 lambda = 1e4/nu."""
    nu = np.asarray(nu, dtype=F64)
    positive = nu > 0.
    lam = (1e4/np.where(positive, nu, 1.))
    short = lam <= paths.RAYLEIGH_SPLIT
    a, b, c, d = (np.where(short, kind(x), kind(y))
                  for x, y in zip(paths.RAYLEIGH_SHORT, paths.RAYLEIGH_LONG))
    lam = lam.astype(kind)
    with np.errstate(all="ignore"):
        e = (b + c*lam) + d/lam
        x = e*np.log(lam)
        sigma = (kind(1e-4)*a)*np.exp(-x)
    return np.where(positive, sigma, kind(0.)), np.where(positive, np.abs(x), kind(0.))


def rayleigh_grid():
    """Wavenumbers from the far infrared to 0.15 um, both rows of the fit, lambda = 0.5 um and
    its neighbours, and nu <= 0."""
    rng = np.random.default_rng(12)
    split = 1e4/paths.RAYLEIGH_SPLIT
    return np.concatenate([[-3., 0.], np.sort(rng.uniform(1., 66000., 1024)),
                           [np.nextafter(split, 0.), split, np.nextafter(split, np.inf)]])


# ---------------------------------------------------------------------------------------------
# The case tables.
# Every loop of path_levels with the eight rows in flight going up (16: two full batches); going
# down one row is in flight and every depth takes the same loop.
DEPTHS = (1, 8, 9, 16, 17)
MU0 = solar.MU0             # (1, 1e-3, 0.25)
ALBEDO = solar.ALBEDO       # (1, 0.3, 0)


def shape_inputs(columns, depth, seed, albedo_rows=False):
    """A problem for the shapes: sweep_cases.Problem's beta (1e-12 .. 10 m-1 with zeros) and
    thicknesses (one of them 0, and its air column with it), air columns that put the Rayleigh
    depth between 0 and ~1, a grey scatterer in two thirds of the levels with omega_c in {0, 1,
    random} and g_c up to 0.9."""
    problem = cases.Problem(columns, depth, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    levels = problem.levels
    sigma = rng.uniform(0., 1e-30, size=columns)
    sigma[::7] = 0.
    air = problem.thickness*rng.uniform(0.2e30, 1e30, size=levels)
    air[rng.random(levels) < 0.2] = 0.
    tau_c = np.where(rng.random(levels) < 0.67, 10.**rng.uniform(-3., 1.5, size=levels), 0.)
    omega_c = rng.choice([0., 1., 0.5, 0.999], size=levels)
    omega_c = np.where(omega_c == 0.5, rng.uniform(0., 1., size=levels), omega_c)
    g_c = rng.choice([0., 0.9, 0.5], size=levels)
    g_c = np.where(g_c == 0.5, rng.uniform(0., 0.9, size=levels), g_c)
    w_c = omega_c*tau_c
    table = np.stack([problem.thickness, air, tau_c, w_c, w_c*g_c], axis=1)
    albedo = ALBEDO
    if albedo_rows:
        albedo = rng.uniform(0., 1., size=(PATHS, columns))
        albedo[0], albedo[2, ::3] = 1., 0.
    return Inputs("shape %d x %d" % (columns, depth), problem.beta, table, MU0,
                  solar.solar_row(problem), sigma, albedo)


def rayleigh_only():
    """No scatterer, 9 levels per path on 67 columns in groups j % 6: 0 beta = 0 (exactly
    conservative); 1 beta = delta*tau_R/s with 1 - omega = delta log-uniform in 1e-13 .. 1e-8, so
    that k2*(1 + t*t) lies on both sides of 1e-10; 2 s*beta >= 800 in each path's first and last
    level; 3 random beta; 4 beta = 0 under a Rayleigh depth near 300 per level (conservative and
    thick); 5 sigma = 0 (pure absorption, omega = 0).  Level 3 of every path has s_l = c_l = 0:
    the identity."""
    rng = np.random.default_rng(21)
    n, columns = 9, 67
    levels = PATHS*n
    group = np.arange(columns) % 6
    thickness = rng.uniform(0.5, 1.5, size=levels)
    air = thickness*rng.uniform(0.5e30, 1e30, size=levels)
    for p in range(PATHS):
        thickness[n*p + 3] = air[n*p + 3] = 0.
    sigma = rng.uniform(0.1e-30, 1e-30, size=columns)
    sigma[group == 4] = 400e-30
    sigma[group == 5] = 0.
    beta = 10.**rng.uniform(-6., 0.5, size=(levels, columns))
    beta[:, (group == 0) | (group == 4)] = 0.
    delta = 10.**rng.uniform(-13., -8., size=(levels, int(np.sum(group == 1))))
    safe = np.where(thickness > 0., thickness, 1.)
    beta[:, group == 1] = delta*(air[:, None]*sigma[None, group == 1])/safe[:, None]
    for p in range(PATHS):
        for level in (n*p, n*p + n - 1):
            beta[level, group == 2] = rng.uniform(800., 3000., size=int(np.sum(group == 2))) / \
                thickness[level]
    zeros = np.zeros(levels)
    table = np.stack([thickness, air, zeros, zeros, zeros], axis=1)
    s = rng.uniform(0.05, 1., size=columns)
    s[-1] = 0.
    inputs = Inputs("rayleigh only", beta, table, MU0, s, sigma, ALBEDO)
    inputs.group = group
    return inputs


def cloud():
    """A grey scatterer in every level but one per path, without Rayleigh scattering in half of
    them: omega_c = 0 and 1 among random ones, g_c up to 0.9, tau_c from 1e-8 to 900; columns in
    groups j % 3: 0 beta = 0, 1 s*beta >= 800 in the first and last level, 2 random."""
    rng = np.random.default_rng(22)
    n, columns = 8, 67
    levels = PATHS*n
    group = np.arange(columns) % 3
    thickness = rng.uniform(0.5, 1.5, size=levels)
    air = np.where(rng.random(levels) < 0.5, thickness*rng.uniform(0.5e30, 1e30, size=levels), 0.)
    sigma = rng.uniform(0.1e-30, 1e-30, size=columns)
    tau_c = 10.**rng.uniform(-8., np.log10(900.), size=levels)
    tau_c[[2, n + 5, 2*n + 7]] = 0.
    tau_c[[1, n + 1]] = 900.
    omega_c = rng.uniform(0., 1., size=levels)
    omega_c[0::4], omega_c[1::4] = 0., 1.
    omega_c[5] = 1. - 1e-16
    g_c = rng.uniform(0., 0.9, size=levels)
    g_c[0::5], g_c[2::5] = 0.9, 0.
    beta = 10.**rng.uniform(-6., 0.5, size=(levels, columns))
    beta[:, group == 0] = 0.
    for p in range(PATHS):
        for level in (n*p, n*p + n - 1):
            beta[level, group == 1] = rng.uniform(800., 2000., size=int(np.sum(group == 1))) / \
                thickness[level]
    w_c = omega_c*tau_c
    table = np.stack([thickness, air, tau_c, w_c, w_c*g_c], axis=1)
    inputs = Inputs("cloud", beta, table, np.array([1., 1e-3, 0.5]),
                    rng.uniform(0.05, 1., size=columns), sigma, np.array([0., 1., 0.3]))
    inputs.group, inputs.omega_c, inputs.g_c = group, omega_c, g_c
    return inputs


RESONANCE_D = (0., 0.9999e-4, -0.9999e-4, 1.0001e-4, -1.0001e-4)
RESONANCE_MU0 = np.array([1., 0.8, 0.6])


def resonance():
    """k*mu0 = 1 + d for d in RESONANCE_D (columns j % 5 of each path's own third of the 15*3
    columns): two levels per path, each a scatterer of tau_c = 1, omega_c = 1, g_c = 0 over an
    absorber s*beta = u/(1 - u), so that w = 1 - u and k2 = 2 u (1.5 + 0.5 u) = ((1 + d)/mu0)^2,
    u = (-3 + sqrt(9 + 4 k2))/2.  The columns of the other paths' thirds lie far from resonance."""
    n, columns = 2, 45
    levels = PATHS*n
    beta = np.zeros((levels, columns))
    d = np.array([RESONANCE_D[j % 5] for j in range(columns)])
    third = np.arange(columns)//15
    for p in range(PATHS):
        k2 = ((1. + d)/RESONANCE_MU0[third])**2
        u = (-3. + np.sqrt(9. + 4.*k2))/2.
        beta[n*p:n*p + n] = (u/(1. - u))[None, :]
    ones, zeros = np.ones(levels), np.zeros(levels)
    table = np.stack([ones, zeros, ones, ones, zeros], axis=1)
    inputs = Inputs("resonance", beta, table, RESONANCE_MU0, np.full(columns, 0.7),
                    np.zeros(columns), np.array([0.3, 0.3, 0.3]))
    inputs.d, inputs.third = d, third
    return inputs


def value_cases():
    return [rayleigh_only(), cloud(), resonance()]


def shape_cases():
    """Every problem the shape tests run: [(inputs, from_last)]."""
    out = []
    for columns in cases.LAYOUT_COLUMNS:
        out.append((shape_inputs(columns, 9, columns), True))
    for depth in DEPTHS:
        for from_last in (False, True):
            out.append((shape_inputs(513, depth, 40 + depth, albedo_rows=True), from_last))
    for _, columns, _ in cases.BAND_SETS:
        out.append((shape_inputs(columns, 3, 70), True))
    return out


def all_cases():
    return shape_cases() + [(inputs, from_last) for inputs in value_cases()
                            for from_last in (False, True)]


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class TwoStreamRecorder(solar.SolarRecorder):
    """tests/solar_cases.py's engine with the two calls of compute_solar_flux."""
    def rayleigh_row(self, grid, row, columns, **keywords):
        self.record("rayleigh_row", grid=grid, row=row, columns=columns,
                    **self._described(keywords))

    def path_two_stream(self, beta, columns, n_paths, levels_per_path, level_begin, level_table,
                        solar_zenith_cosine, solar_row, work, **keywords):
        self.record("path_two_stream", beta=beta, columns=columns, n_paths=n_paths,
                    levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table),
                    solar_zenith_cosine=np.asarray(solar_zenith_cosine), solar_row=solar_row,
                    work=work, **self._described(keywords))


@contextlib.contextmanager
def recorded(directory):
    """surface_cases.recorded with a TwoStreamRecorder."""
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = TwoStreamRecorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before
