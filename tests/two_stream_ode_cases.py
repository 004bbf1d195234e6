"""What tests/test_two_stream_ode_host.py (CPU) and tests/test_gpu_two_stream_ode.py (GPU) share:
a reference of the two-stream products that knows the two-stream *equations* and none of their
closed forms, in numpy long double, and the case tables of the GPU tests.

The equations, with tau increasing away from space, I+ upward and I- downward:

    solar (F0 = 1, s = exp(-tau/mu0)):
        dI+/dtau = g1*I+ - g2*I- - (w*g3/mu0)*s
        dI-/dtau = g2*I+ - g1*I- + (w*g4/mu0)*s
        g2 = 3*w*(1 - gp)/4 ; dif = 2*(1 - w) ; g1 = g2 + dif ; g3 = (2 - 3*mu0*gp)/4 ; g4 = 1 - g3
    thermal:
        dI+/dtau = g1*I+ - g2*I- - dif*B(tau)
        dI-/dtau = g2*I+ - g1*I- + dif*B(tau)
        g2 = D*w*(1 - gp)/2 ; dif = D*(1 - w) ; g1 = g2 + dif
        B(tau) = B (isothermal) or Bt + (Bb - Bt)*tau/t (linear source)

A layer is an operator between what enters it and what leaves it: reflection from above and from
below, what it absorbs of either (the rest is transmitted), and what its sources send out of its
top and its bottom.  The
operator of a sublayer of thickness h = t/2^n, ||M||*h <= 1/16, comes from the power series of the
propagator exp(M*h) of the equations written as one autonomous linear system (the sources are
extra states: s with s' = -s/mu0; a constant; tau with tau' = 1); the layer is that sublayer
doubled n times with the star product of two layers, which stays stable where a propagator of the
whole layer cancels.  A column is the linear system in its 2(L + 1) interface fluxes -- the two
relations of every layer, no light from space, and the surface -- solved by elimination with
partial pivoting.  Nothing here is a Meador-Weaver expression, has a k or a branch, or follows
the adding recurrences of the kernels.

The layer's inputs (t, w, gp, mu0 or D) are the float64 ones of the mirrors' layer_inputs: the
same hand-over the long-double mirrors use, which keeps the rounding of the inputs out of every
comparison.  A shortwave layer in the resonance guard is solved at its own mu0.

The constants below are what tests/test_two_stream_ode_host.py measures, each beside the measured
figure; that file asserts measured <= CONSTANT <= 2*measured for every one of them."""
import numpy as np

from tests import scatterer_cases as spectral
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_source_cases as tsc
from tests import two_stream_cases as ts

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
SERIES_NORM = 16            # ||M||*h <= 1/SERIES_NORM
SERIES_TERMS = 12           # (1/16)^13/14! = 2^-88: nothing is left of the series' tail
GUARD = ts.RESONANCE

# ---------------------------------------------------------------------------------------------
# What was measured.
# The reference against 60-digit mpmath (matrix exponentials of single layers from t = 1e-3 to
# 1e3, and 3-level columns by LU), absolute in units of F0 = 1 or B = 1.  The bound is reasoned:
# at most 30 doublings (||M||*t <= 2^26), each a sum of positive terms none above 1 that adds a
# rounding or two of 2^-64 to what it carries: 64*2^-64 = 3.5e-18.
REFERENCE_ERROR = 2.5e-19   # measured 2.44e-19 (layers 2.18e-19 and 2.44e-19, columns 1.86e-19)
REFERENCE_BOUND = 64.*2.**-64

# |long-double mirror - reference| of single layers over the case tables of the mirrors and of
# this file, by the mirror's branch, in units of F0 = 1 (Rdif, Tdif, Rdir, Tdp) or B = 1 (R, T,
# em; with the linear source S_up and S_dn under (Bt, Bb) = (0, 1) and (1, 0)).  The general
# shortwave figure is the mirror's own rounding in the columns that two_stream_cases.resonance()
# puts 1e-8 outside the guard, where the quotient by (1 - x)*(1 + x) amplifies it by 1e4.
SOLAR_LAYER = {"identity": 0.,              # measured 0
               "conservative": 4.8e-11,     # measured 4.78e-11
               "general": 6.6e-15,          # measured 6.54e-15
               "guarded": 1.19e-5}          # measured 1.180e-5
THERMAL_LAYER = {"clear": 3.8e-19,          # measured 3.79e-19
                 "conservative": 4.1e-11,   # measured 4.07e-11
                 "general": 5.5e-19}        # measured 5.42e-19
SOURCE_LAYER = {"clear": 4.9e-19,           # measured 4.88e-19
                "conservative": 2.0e-11,    # measured 1.98e-11
                "general": 6.6e-19}         # measured 6.56e-19
# The same of whole columns over the mirrors' own case tables (two_stream_cases' and, for both
# longwave sources, thermal_source_cases', which are thermal_cases' with interface temperatures
# beside them): every flux at every interface, relative to F0 or to the thermal scale.  A column
# counts under the last of these classes that one of its levels takes (see solar_column_class).
# What a level's cut costs adds up along a column and grows with the light that passes a level
# more than once.
SOLAR_COLUMN = {"general": 7.5e-15,         # measured 7.40e-15
                "conservative": 3.6e-10,    # measured 3.56e-10
                "guarded": 1.27e-5}         # measured 1.2697e-5
THERMAL_COLUMN = {"clear": 2.5e-19,         # measured 2.45e-19
                  "general": 3.0e-18,       # measured 2.94e-18
                  "conservative": 1.57e-10}  # measured 1.566e-10
SOURCE_COLUMN = {"clear": 3.6e-19,          # measured 3.55e-19
                 "general": 3.0e-18,        # measured 2.94e-18
                 "conservative": 1.57e-10}  # measured 1.566e-10
# The same over the tables of this file alone, which the GPU tests run: what their bounds add.
# Every level of the conservative tables' odd columns has omega = 1 - 1e-11, up to 17 of them on
# top of each other over A = 1.
SOLAR_TABLES = {"general": 3.3e-15,         # measured 3.24e-15
                "conservative": 2.25e-9,    # measured 2.241e-9
                "guarded": 1.28e-5}         # measured 1.2732e-5
THERMAL_TABLES = {"clear": 2.9e-19,         # measured 2.81e-19
                  "general": 3.2e-18,       # measured 3.19e-18
                  "conservative": 2.19e-9}  # measured 2.182e-9
SOURCE_TABLES = {"clear": 3.0e-19,          # measured 2.99e-19
                 "general": 3.2e-18,        # measured 3.14e-18
                 "conservative": 1.83e-9}   # measured 1.827e-9
# Section 25's conservative em against the reference, as a fraction of the estimate k2*t*t/2.
EM_FRACTION = 0.993         # measured 0.9928
# The resonance guard alone: the worst error of Rdir and Tdp over the scan of
# tests/test_two_stream_ode_host.py (g_c up to 0.9, the Sun down from the zenith, where it is
# worst), and the slope c of error <= c*(1e-4 - |1 - k*mu0|).
GUARD_ERROR = 1.2e-5        # measured 1.196e-5 (t = 0.562, w = 0.605, gp = 0.474, mu0 = 1, k*mu0 = 1)
GUARD_SLOPE = 0.12          # measured 0.1196


# ---------------------------------------------------------------------------------------------
# A layer as an operator.
class Operator(object):
    """rt and rb: reflection of light from above and from below; at and ab: what the layer absorbs
    of light from above and from below; up and dn [sources, ...]: what each unit source sends out
    of the top and the bottom.  What is transmitted is what is neither reflected nor absorbed.

    The absorbed part is carried, not the transmitted one: a sublayer of a nearly conservative
    layer absorbs far less than a rounding of its transmittance, and a thick layer is made of
    millions of them."""
    def __init__(self, rt, rb, at, ab, up, dn):
        self.rt, self.rb, self.at, self.ab, self.up, self.dn = rt, rb, at, ab, up, dn
        self.td, self.tu = (LD(1.) - rt) - at, (LD(1.) - rb) - ab

    def parts(self):
        return self.rt, self.rb, self.at, self.ab, self.up, self.dn

    def where(self, mask, other):
        return Operator(*(np.where(mask, a, b) for a, b in zip(self.parts(), other.parts())))


def star(a, b):
    """The layer made of a (nearer space) on top of b.  Between the two, light that entered a from
    above goes down as a.td*m and up as b.rt*(a.td*m), m = 1/(1 - a.rb*b.rt): each layer absorbs
    its part of either; and so for light from below, and for the sources."""
    one = LD(1.)
    m = one/(one - a.rb*b.rt)
    return Operator(a.rt + a.tu*(b.rt*(a.td*m)), b.rb + b.td*(a.rb*(b.tu*m)),
                    a.at + (a.td*m)*(b.at + b.rt*a.ab), b.ab + (b.tu*m)*(a.ab + a.rb*b.at),
                    a.up + a.tu*((b.up + b.rt*a.dn)*m), b.dn + b.td*((a.dn + a.rb*b.up)*m))


def integral(matrix):
    """phi(matrix) = sum_k matrix^k/(k + 1)! for matrix [..., n, n] of small norm, summed from
    its tail: exp(matrix) = 1 + matrix phi(matrix), and the integral of exp(M s) over a sublayer
    of thickness h is h phi(M h)."""
    eye = np.broadcast_to(np.eye(matrix.shape[-1], dtype=LD), matrix.shape)
    phi = eye
    for k in range(SERIES_TERMS, 0, -1):
        phi = eye + np.matmul(matrix, phi)/LD(k + 1)
    return phi


def sublayer(matrix, h, dif, sources):
    """The operator of a sublayer so thin that the power series of its propagator p = exp(M h)
    is exact to rounding: with y = (I+, I-, source states...) and y(h) = p y(0), I+(0) and I-(h)
    follow from I-(0) and I+(h).  Source i is the state 2 + i at 1 (the others at 0) on top of the
    sublayer.  What is absorbed comes from the equations' own balance, d(I+ - I-)/dtau =
    dif*(I+ + I-) without sources: I+ - I- changes over the sublayer by dif*h*(1, 1) phi(M h) y(0),
    a sum of positive terms."""
    one = LD(1.)
    a = matrix*h[..., None, None]
    phi = integral(a)
    e = np.matmul(a, phi)                                           # p - 1
    tu = one/(one + e[..., 0, 0])
    rt = -e[..., 0, 1]*tu
    rb = e[..., 1, 0]*tu
    gain = dif*h
    at = gain*((phi[..., 0, 0] + phi[..., 1, 0])*rt + (phi[..., 0, 1] + phi[..., 1, 1]))
    ab = gain*((phi[..., 0, 0] + phi[..., 1, 0])*tu)
    up = np.stack([-e[..., 0, 2 + i]*tu for i in range(sources)])
    dn = np.stack([e[..., 1, 2 + i] for i in range(sources)]) + e[..., 1, 0]*up
    return Operator(rt, rb, at, ab, up, dn)


def doubled(matrix, t, dif, sources, lower):
    """The operator of a layer of thickness t [...] under y' = matrix y (matrix [..., n, n], of
    which (1, -1) times the block of I+ and I- is dif*(1, 1)); lower(op, H): the sources of op as
    they are H further from space."""
    with np.errstate(all="ignore"):
        norm = np.max(np.sum(np.abs(matrix), axis=-1), axis=-1)
        size = (norm*t*LD(SERIES_NORM)).astype(F64)
        n = np.where(size > 1., np.ceil(np.log2(np.where(size > 1., size, 1.))), 0.).astype(int)
        h = t/LD(2.)**n
        op = sublayer(matrix, h, dif, sources)
        for j in range(int(np.max(n, initial=0))):
            below = lower(op, h*LD(2.)**j)
            op = star(op, Operator(op.rt, op.rb, op.at, op.ab, *below)).where(j < n, op)
    return op


def _matrix(shape, n):
    return np.zeros(shape + (n, n), dtype=LD)


def solar_layer(inputs):
    """(Rdif, Tdif, Rdir, Tdp, D) in long double from layer_inputs' float64 t, w, gp and mu0."""
    # Where tau is 0 the mirrors' omega is 0/0: a layer of no thickness, whatever is in it.
    empty = np.asarray(inputs["tau"]) == 0.
    t, w, gp, mu0 = (np.where(empty & (name != "mu0"), 0., np.asarray(inputs[name], dtype=F64))
                     .astype(LD) for name in ("t", "w", "gp", "mu0"))
    one, two, three, four = LD(1.), LD(2.), LD(3.), LD(4.)
    g2 = three*w*(one - gp)/four
    g1 = g2 + two*(one - w)
    g3 = (two - three*mu0*gp)/four
    g4 = one - g3
    m = _matrix(t.shape, 3)
    m[..., 0, 0], m[..., 0, 1], m[..., 0, 2] = g1, -g2, -(w*g3)/mu0
    m[..., 1, 0], m[..., 1, 1], m[..., 1, 2] = g2, -g1, (w*g4)/mu0
    m[..., 2, 2] = -one/mu0

    def lower(op, thickness):
        beam = np.exp(-thickness/mu0)
        return beam*op.up, beam*op.dn
    op = doubled(m, t, two*(one - w), 1, lower)
    with np.errstate(all="ignore"):
        return op.rt, op.td, op.up[0], op.dn[0], np.exp(-t/mu0)


def thermal_layer(inputs):
    """(R, T, em, up1, dn1) in long double from thermal_cases.layer_inputs' float64 t, w, gp and
    D: em leaves either face under B = 1, up1 and dn1 leave the top and the bottom under
    B(tau) = tau/t (0 for t = 0)."""
    t, w, gp = (np.asarray(inputs[name], dtype=F64).astype(LD) for name in ("t", "w", "gp"))
    d = LD(inputs["d"])
    one, two = LD(1.), LD(2.)
    g2 = d*w*(one - gp)/two
    dif = d*(one - w)
    g1 = g2 + dif
    # States: I+, I-, c (constant: B = c), u (constant: tau' = u) and tau (B = tau).
    m = _matrix(t.shape, 5)
    m[..., 0, 0], m[..., 0, 1], m[..., 0, 2], m[..., 0, 4] = g1, -g2, -dif, -dif
    m[..., 1, 0], m[..., 1, 1], m[..., 1, 2], m[..., 1, 4] = g2, -g1, dif, dif
    m[..., 4, 3] = one

    def lower(op, thickness):
        # B = tau of the whole is thickness + tau of the lower half.
        return (np.stack([op.up[0], thickness*op.up[0] + op.up[1]]),
                np.stack([op.dn[0], thickness*op.dn[0] + op.dn[1]]))
    op = doubled(m, t, dif, 2, lower)
    safe = np.where(t > 0., t, one)
    return op.rt, op.td, op.up[0], np.where(t > 0., op.up[1]/safe, 0.), \
        np.where(t > 0., op.dn[1]/safe, 0.)


# ---------------------------------------------------------------------------------------------
# A column as one linear system.
def solve(a, b):
    """x of a x = b for a [E, n, n] and b [E, n] in long double: elimination with partial
    pivoting, every system at once."""
    a, b = np.array(a, dtype=LD), np.array(b, dtype=LD)
    count, n = b.shape
    each = np.arange(count)
    for k in range(n):
        pivot = k + np.argmax(np.abs(a[:, k:, k]), axis=1)
        row, rhs = a[each, pivot].copy(), b[each, pivot].copy()
        a[each, pivot], b[each, pivot] = a[:, k], b[:, k]
        a[:, k], b[:, k] = row, rhs
        factor = a[:, k + 1:, k]/a[:, k, k][:, None]
        a[:, k + 1:, k:] -= factor[:, :, None]*a[:, None, k, k:]
        b[:, k + 1:] -= factor*b[:, k][:, None]
    x = np.zeros_like(b)
    for k in range(n - 1, -1, -1):
        x[:, k] = (b[:, k] - np.sum(a[:, k, k + 1:]*x[:, k + 1:], axis=1))/a[:, k, k]
    return x


def interface_fluxes(rt, rb, td, tu, s_up, s_dn, reflectance, surface_source):
    """(I+, I-) at the L + 1 interfaces [L + 1, ...] of L layers (each argument [L, ...], the
    nearest to space first): for every layer i
        I+[i] = rt_i I-[i] + tu_i I+[i+1] + s_up_i ; I-[i+1] = td_i I-[i] + rb_i I+[i+1] + s_dn_i
    with I-[0] = 0 and I+[L] = reflectance*I-[L] + surface_source (both [...])."""
    levels, shape = rt.shape[0], rt.shape[1:]
    flat = [np.reshape(np.broadcast_to(x, rt.shape), (levels, -1)) for x in
            (rt, rb, td, tu, s_up, s_dn)]
    rt, rb, td, tu, s_up, s_dn = flat
    reflectance = np.reshape(np.broadcast_to(reflectance, shape), -1)
    surface_source = np.reshape(np.broadcast_to(surface_source, shape), -1)
    count, n = rt.shape[1], 2*(levels + 1)
    a, b = np.zeros((count, n, n), dtype=LD), np.zeros((count, n), dtype=LD)
    up, dn = (lambda i: i), (lambda i: levels + 1 + i)
    for i in range(levels):
        a[:, 2*i, up(i)], a[:, 2*i, dn(i)], a[:, 2*i, up(i + 1)] = 1., -rt[i], -tu[i]
        b[:, 2*i] = s_up[i]
        a[:, 2*i + 1, dn(i + 1)], a[:, 2*i + 1, dn(i)], a[:, 2*i + 1, up(i + 1)] = \
            1., -td[i], -rb[i]
        b[:, 2*i + 1] = s_dn[i]
    a[:, n - 2, dn(0)] = 1.
    a[:, n - 1, up(levels)], a[:, n - 1, dn(levels)] = 1., -reflectance
    b[:, n - 1] = surface_source
    x = solve(a, b)
    return (x[:, :levels + 1].T.reshape((levels + 1,) + shape),
            x[:, levels + 1:].T.reshape((levels + 1,) + shape))


def solar_column(layers, albedo, f0):
    """{"up", "down", "direct", "diffuse"} [L + 1, ...] from solar_layer's tuple of L levels in
    the Sun's order [L, ...], the albedo and F0 [...]."""
    rdif, tdif, rdir, tdp, d = layers
    albedo = np.asarray(albedo, dtype=F64).astype(LD)
    f0 = np.asarray(f0, dtype=F64).astype(LD)
    direct = np.ones((rdif.shape[0] + 1,) + rdif.shape[1:], dtype=LD)
    for i in range(rdif.shape[0]):
        direct[i + 1] = direct[i]*d[i]
    up, diffuse = interface_fluxes(rdif, rdif, tdif, tdif, rdir*direct[:-1], tdp*direct[:-1],
                                   albedo, albedo*direct[-1])
    out = {"up": f0*up, "diffuse": f0*diffuse, "direct": f0*direct}
    out["down"] = out["direct"] + out["diffuse"]
    return out


def thermal_column(layers, bt, bb, emissivity, surface_b):
    """{"up", "down"} [L + 1, ...] from thermal_layer's tuple of L levels in the order space ->
    surface, pi*B at each level's space-side and surface-side face [L, ...] (the same for an
    isothermal level), eps and pi*B(T_s) [...]."""
    r, t, em, up1, dn1 = layers
    eps = np.asarray(emissivity, dtype=F64).astype(LD)
    db = bb - bt
    up, down = interface_fluxes(r, r, t, t, bt*em + db*up1, bt*em + db*dn1, LD(1.) - eps,
                                eps*surface_b)
    return {"up": up, "down": down}


def _flat(inputs, order, result, names):
    """The mirrors' layout: every quantity [levels, columns] at the interface below each flat
    level, "top_" + quantity [PATHS, columns] at interface 0."""
    out = {}
    for q in names:
        below = np.zeros((inputs.levels, inputs.columns), dtype=LD)
        below[order] = result[q][1:]
        out[q], out["top_" + q] = below, result[q][0]
    return out


def solar_reference(inputs, from_last, layers=None):
    """two_stream_cases.mirror's dict from the equations (inputs: a two_stream_cases.Inputs or a
    scatterer_cases.Shortwave; layers: solar_layer of its layer_inputs(from_last), if at hand)."""
    albedo = inputs.albedo[:, None] if inputs.albedo.ndim == 1 else inputs.albedo
    f0 = inputs.f0()
    if layers is None:
        layers = solar_layer(inputs.layer_inputs(from_last))
    result = solar_column(layers, albedo, f0)
    out = _flat(inputs, inputs.sun_order(from_last).T, result, ts.QUANTITIES)
    out["f0"] = f0
    return out


def thermal_reference(inputs, from_last, linear, layers=None):
    """thermal_cases.mirror's (the level temperatures) or thermal_source_cases.mirror's (linear:
    the interface temperatures of a thermal_source_cases.Inputs) "up", "down", their "top_" rows
    and "scale", from the equations (layers: thermal_layer of its layer_inputs(from_last), if at
    hand)."""
    order = inputs.order(from_last).T                               # [L, PATHS]
    eps = inputs.emissivity[:, None] if inputs.emissivity.ndim == 1 else inputs.emissivity
    nu = inputs.nu[None, None, :]
    if linear:
        space = 1 if from_last else 0
        edges = inputs.edges[order]                                 # [L, PATHS, 2]
        bt = tc.pi_planck(LD, nu, edges[:, :, space, None])
        bb = tc.pi_planck(LD, nu, edges[:, :, 1 - space, None])
        scale = inputs.scale()
    else:
        bt = bb = tc.pi_planck(LD, nu, inputs.table[order][:, :, None, 4])
        scale = inputs.isothermal().scale() if hasattr(inputs, "edges") else inputs.scale()
    surface_b = tc.pi_planck(LD, inputs.nu[None, :], inputs.surface_t[:, None])
    if layers is None:
        layers = thermal_layer(inputs.layer_inputs(from_last))
    result = thermal_column(layers, bt, bb, eps, surface_b)
    out = _flat(inputs, order, result, tc.QUANTITIES)
    out["scale"] = scale
    return out


# ---------------------------------------------------------------------------------------------
# Which branches of the mirror a table takes.  Where k2 is exactly 0 the conservative branch is
# no cut but the limit itself: such a level counts as general (as exact), so that a column counts
# as conservative only where something was neglected.  The class of a column thus follows from the
# float64 layer inputs and the criteria the definition states, as the mirror forms them: it only
# says where a documented cut applies, and so which recorded constant a bound may add.
SOLAR_CLASSES = ("general", "conservative", "guarded")
THERMAL_CLASSES = ("clear", "general", "conservative")


def solar_column_class(li):
    """[PATHS, columns] from layer_inputs' arrays [L, PATHS, columns]: the index in SOLAR_CLASSES
    that a column counts under, the last that one of its levels takes."""
    cut = (li["branch"] == ts.CONSERVATIVE_BRANCH) & (li["k2"] > 0.)
    return np.where(np.any(li["branch"] == ts.GUARDED, axis=0), 2,
                    np.where(np.any(cut, axis=0), 1, 0))


def thermal_column_class(li):
    """The same in THERMAL_CLASSES."""
    cut = (li["branch"] == tc.CONSERVATIVE_BRANCH) & (li["k2"] > 0.)
    return np.where(np.any(cut, axis=0), 2,
                    np.where(np.any(li["branch"] != tc.CLEAR, axis=0), 1, 0))


def guarded_elements(inputs, from_last=False):
    """How many elements of a shortwave problem lie in the resonance guard."""
    return int(np.count_nonzero(inputs.layer_inputs(from_last)["branch"] == ts.GUARDED))


def column_allowance(recorded, classes, column_class):
    """[PATHS, columns]: what the long-double mirror may differ from the equations in each
    column, the recorded constant of the column's class."""
    return np.array([recorded[name] for name in classes], dtype=LD)[column_class]


# ---------------------------------------------------------------------------------------------
# The case tables of the GPU tests.
DEPTHS = (1, 2, 9, 17)      # one level, an interior interface, past one and two groups of eight
COLUMNS = (1, 64, 130)      # a lone lane, a full wavefront, two wavefronts and a partial one
LAYOUTS = ("aligned", "odd")
LID = 1000.                 # s*beta of an opaque lid
SURFACE_T = (270., 288., 305.)


def _special(depth):
    """The flat levels (one per path) that are empty (tau = 0, path 0), clear (no scatterer,
    path 1) and, in the columns j % 3 == 1 of path 2, opaque: a lid at either end of the path,
    so that it faces space in both storage orders."""
    at = min(1, depth - 1)
    return at, depth + at, (2*depth, 3*depth - 1)


def _scatterer(rng, levels, g_max):
    """tau_c from 1e-3 to 50, omega_c from 0.05 to 1 - 1e-6 and g_c up to g_max, with each of the
    ends among the levels where there are enough of them."""
    tau_c = 10.**rng.uniform(-3., np.log10(50.), size=levels)
    omega_c = rng.uniform(0.05, 1. - 1e-6, size=levels)
    g_c = rng.uniform(0., g_max, size=levels)
    if levels >= 6:
        tau_c[[2, levels - 1]] = 1e-3, 50.
        omega_c[[0, levels - 2]] = 0.05, 1. - 1e-6
        g_c[[2, levels - 3]] = 0., g_max
    return tau_c, omega_c, g_c


def _absorber(rng, levels, columns):
    """beta from 1e-6 to 3 m-1, and none at all in every seventh column."""
    beta = 10.**rng.uniform(-6., 0.5, size=(levels, columns))
    beta[:, 5::7] = 0.
    return beta


def solar_general(columns, depth):
    """A grey scatterer in every level over a random absorber and Rayleigh scattering in half of
    the levels, with _special's levels, under mu0 = (1, 1e-3, 0.25) and A = (1, 0.3, 0)."""
    rng = np.random.default_rng(5000 + 100*depth + columns)
    levels = PATHS*depth
    thickness = rng.uniform(0.5, 1.5, size=levels)
    air = np.where(rng.random(levels) < 0.5, thickness*rng.uniform(0.2e30, 1e30, size=levels), 0.)
    sigma = rng.uniform(0., 1e-30, size=columns)
    tau_c, omega_c, g_c = _scatterer(rng, levels, 0.9)
    beta = _absorber(rng, levels, columns)
    empty, clear, lids = _special(depth)
    thickness[empty] = air[empty] = tau_c[empty] = 0.
    air[clear] = tau_c[clear] = 0.
    for level in lids:
        beta[level, 1::3] = LID/thickness[level]
    w_c = omega_c*tau_c
    table = np.stack([thickness, air, tau_c, w_c, w_c*g_c], axis=1)
    return ts.Inputs("general %d x %d" % (columns, depth), beta, table, ts.MU0,
                     rng.uniform(0.05, 1., size=columns), sigma, ts.ALBEDO)


def solar_conservative(columns, depth):
    """Scatterers of omega_c = 1 and nothing else: over no absorber in the even columns (omega =
    1 exactly), over s*beta = 1e-11*tau_c in the odd ones (omega = 1 - 1e-11, on either side of
    the conservative cut as tau_c goes from 1e-3 to 50); path 0 has A = 1 under mu0 = 1."""
    rng = np.random.default_rng(6000 + 100*depth + columns)
    levels = PATHS*depth
    thickness = rng.uniform(0.5, 1.5, size=levels)
    tau_c, _, g_c = _scatterer(rng, levels, 0.9)
    beta = np.zeros((levels, columns))
    beta[:, 1::2] = (1e-11*tau_c/thickness)[:, None]
    zeros = np.zeros(levels)
    table = np.stack([thickness, zeros, tau_c, tau_c, tau_c*g_c], axis=1)
    inputs = ts.Inputs("conservative %d x %d" % (columns, depth), beta, table, ts.MU0,
                       rng.uniform(0.05, 1., size=columns), np.zeros(columns), ts.ALBEDO)
    inputs.exact = np.arange(columns) % 2 == 0
    return inputs


def solar_guard(columns, depth):
    """two_stream_cases.resonance() at any shape: k*mu0 = 1 + d for d of RESONANCE_D in the
    columns j % 5, under mu0 = (1, 0.8, 0.6); every level a scatterer of tau_c = 1, omega_c = 1,
    g_c = 0 over the absorber that puts k there."""
    levels = PATHS*depth
    d = np.array([ts.RESONANCE_D[j % 5] for j in range(columns)])
    beta = np.zeros((levels, columns))
    for p in range(PATHS):
        k2 = ((1. + d)/ts.RESONANCE_MU0[p])**2
        u = (-3. + np.sqrt(9. + 4.*k2))/2.
        beta[depth*p:depth*(p + 1)] = (u/(1. - u))[None, :]
    ones, zeros = np.ones(levels), np.zeros(levels)
    table = np.stack([ones, zeros, ones, ones, zeros], axis=1)
    inputs = ts.Inputs("guard %d x %d" % (columns, depth), beta, table, ts.RESONANCE_MU0,
                       np.full(columns, 0.7), np.zeros(columns), np.array([0.3, 1., 0.]))
    inputs.d = d
    return inputs


def _thermal(name, rng, columns, depth, beta, thickness, tau_c, w_c, g_c):
    levels = PATHS*depth
    temperature = rng.uniform(180., 320., size=levels)
    interfaces = rng.uniform(150., 320., size=(PATHS, depth + 1))
    table = np.stack([thickness, tau_c, w_c, g_c, temperature], axis=1)
    nu = np.linspace(1., 3000., columns) if columns > 1 else np.array([667.])
    return tsc.Inputs("%s %d x %d" % (name, columns, depth), nu, beta, table, interfaces,
                      SURFACE_T, tc.EMISSIVITY)


def thermal_general(columns, depth):
    """solar_general's scatterers, absorber and special levels for the longwave entries, with
    level temperatures from 180 to 320 K and interface temperatures from 150 to 320 K (inversions
    among them) under eps = (1, 0.3, 0): a thermal_source_cases.Inputs, whose isothermal() the
    entry of the level temperatures takes."""
    rng = np.random.default_rng(7000 + 100*depth + columns)
    levels = PATHS*depth
    thickness = rng.uniform(0.5, 1.5, size=levels)
    tau_c, omega_c, g_c = _scatterer(rng, levels, 0.9)
    beta = _absorber(rng, levels, columns)
    empty, clear, lids = _special(depth)
    thickness[empty] = tau_c[empty] = 0.
    omega_c[clear] = 0.
    for level in lids:
        beta[level, 1::3] = LID/thickness[level]
    return _thermal("general", rng, columns, depth, beta, thickness, tau_c, omega_c*tau_c, g_c)


def thermal_conservative(columns, depth):
    """solar_conservative for the longwave entries."""
    rng = np.random.default_rng(8100 + 100*depth + columns)
    levels = PATHS*depth
    thickness = rng.uniform(0.5, 1.5, size=levels)
    tau_c, _, g_c = _scatterer(rng, levels, 0.9)
    beta = np.zeros((levels, columns))
    beta[:, 1::2] = (1e-11*tau_c/thickness)[:, None]
    return _thermal("conservative", rng, columns, depth, beta, thickness, tau_c, tau_c, g_c)


SPECTRAL_SHAPE = (130, 9, 3, 11)    # columns, depth, knots and seed of the two spectral cases


def spectral_shortwave():
    """scatterer_cases.shortwave_inputs with three knots: tau_c, omega_c and g_c differ from
    column to column within a level."""
    return spectral.shortwave_inputs(*SPECTRAL_SHAPE)


def spectral_longwave():
    return spectral.longwave_inputs(*SPECTRAL_SHAPE)


def shapes():
    return [(columns, depth) for depth in DEPTHS for columns in COLUMNS]


def tight_solar_tables():
    """Every shortwave problem that the GPU tests hold to the bound without the guard."""
    return [make(columns, depth) for make in (solar_general, solar_conservative)
            for columns, depth in shapes()] + [spectral_shortwave()]


def guard_tables():
    return [solar_guard(columns, depth) for columns, depth in shapes()]


def thermal_tables():
    """Every longwave problem of the GPU tests (each run with both sources)."""
    return [make(columns, depth) for make in (thermal_general, thermal_conservative)
            for columns, depth in shapes()] + [spectral_longwave()]
