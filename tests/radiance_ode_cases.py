"""What tests/test_radiance_ode_host.py (CPU) and tests/test_gpu_radiance_ode.py (GPU) share: a
reference of the five view products (compute_thermal_radiance, compute_thermal_radiance_linear,
compute_thermal_radiance_at, compute_solar_radiance and the two spectral radiance entries) that
knows the *equations* and none of their closed forms, in numpy long double on top of
tests/two_stream_ode_cases.py, the view cases of the GPU tests, and what was measured.

The equations.  The fluxes I+ and I- are two_stream_ode_cases' (solar; thermal with an isothermal
level; thermal with a source linear in tau).  Along the view, tau' measured from the space-side
face of a level of scaled thickness t, with the cosine mu:

    upward ray   (looking down):   mu dI/dtau' = I - J+(tau'), I given at the surface-side face
    downward ray (looking up):    -mu dI/dtau' = I - J-(tau'), I given at the space-side face

    longwave:  J+- = B(tau') + (w/(2 pi))*[f_with*(1 + a) + f_against*(1 - a)]
               f = F - pi*B(tau') ; a = 3*gp*mu/2 ; with: the flux that travels with the ray
               that is  pi*J+- = (1 - w)*pi*B(tau') + (w/2)*[F_with*(1 + a) + F_against*(1 - a)]
               B constant in the level or linear in tau' between its face values
    shortwave: J+ = (w/(2 pi))*[F+*(1 + a) + F-*(1 - a)]
                    + ((omega/sc)*Pmix/(4 pi))*(S_i/mu0)*exp(-tau'/mu0)
               Pmix = (tau_R*PR + w_c*PH)/tau_s ; PR = (3/4)(1 + cosT^2)
               PH = (1 - gc^2)/(1 + gc^2 - 2 gc cosT)^(3/2)
    surface:   I_L = eps*B(T_s) + (1 - eps)*down[L]/pi ; I_L = A*(direct[L] + diffuse[L])/pi
    space:     I = 0 at interface 0 for the downward ray

A clear longwave level has w = 0 and t = tau, so that J = B; a level of tau = 0 has t = 0 and is
the identity; a shortwave level with tau_s = 0 has w = 0 and omega/sc = 0 and only attenuates.
None of these is a branch here: they are what the equations give for those inputs.

J is linear in the states two_stream_ode_cases' solver already carries (I+, I-, the beam, the
constant and tau), so pi*I along either ray is one more state of the same autonomous linear
system: a one-way stream that is transmitted with exp(-t/mu), is fed by the other states and
feeds none of them.  A layer is therefore a View: two_stream_ode_cases' Operator of the fluxes
and, for each ray, its transmittance and what I- entering the top, I+ entering the bottom and
every unit source contribute to pi*I leaving the exit face.  The View of a sublayer comes from
the same power series of the propagator, the layer from the same doubling (sums of positive
terms, with what a layer takes out of a ray carried in place of its transmittance: stable and
exact to rounding where t/mu reaches 20 000), and a column from
the interface fluxes that two_stream_ode_cases.interface_fluxes solves, one layer's relation per
level.  Nothing here is a closed form of the view, has a k or a branch of the kernels, or uses
their exchanged arguments or the linear source's shift.

The inputs (t, w, gp, mu0 or D, omega/sc, tau_R, tau_s, w_c, gc, cosT) are the float64 ones of the
mirrors' layer_inputs and view_inputs: the hand-over two_stream_ode_cases uses.  A shortwave level
in the resonance guard is solved at its own mu0.

The chain that is measured against this reference is the long-double flux mirror feeding the
long-double view mirror.  The view mirrors read their flux rows as float64, as the kernels do, so
the chain carries one float64 rounding of every flux row: 2^-53 of the flux scale times the
view's gain.  "Rounding level" below is that figure, not 2^-64.

The constants below are what tests/test_radiance_ode_host.py measures, each beside the measured
figure; that file asserts measured <= CONSTANT <= 2*measured for every one of them."""
import functools

import numpy as np

from tests import scatterer_radiance_cases as spectral_view
from tests import solar_radiance_cases as svc
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_radiance_observer_cases as oc
from tests import thermal_radiance_source_cases as rsc
from tests import thermal_source_cases as tsc
from tests import two_stream_cases as ts
from tests import two_stream_ode_cases as ode

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
MU = np.array(rc.MU)                # (1, 0.6, 0.05), one per path
PHI = np.array(svc.PHI)             # (0, 90, 180)
PRODUCTS = ("isothermal", "linear", "solar")

# ---------------------------------------------------------------------------------------------
# What was measured (tests/test_radiance_ode_host.py).
# The reference against 60-digit mpmath: single levels, t from 1e-3 to 1e3 at mu = 1, 0.6 and 0.05,
# both rays and every source, and 3-level columns.  On the mpmath side a level is the matrix
# exponential of the augmented system (beyond growth*t = 40 equal parts of the level by theirs,
# put on top of each other at 60 digits: t/mu = 20 000 in one piece would take 17 000 digits), and
# up to t = 1 that side is itself held to the direct quadrature of the transfer integral over the
# fluxes inside the level (it agrees to 2.9e-62).  Absolute, in units of pi*I under a unit of what
# enters the level or of pi*B, and of the beam's term of pi*J where that exceeds 1.  The bound is
# reasoned as two_stream_ode_cases.REFERENCE_BOUND is: the flux operator that feeds the ray has
# that bound; on top of it at most 30 doublings (||M||*t <= 2^26, ||M|| <= 5 + 1/mu), each of
# which forms a ray's share from sums of positive terms none above 1 in 8 rounded operations.
REFERENCE_ERROR = 4.5e-19   # measured 4.45e-19 (levels 3.40e-19 and 4.45e-19, columns 1.99e-19)
REFERENCE_BOUND = ode.REFERENCE_BOUND + 30.*8.*2.**-64

# |long-double mirror chain - reference|/scale per product and per class of the column
# (two_stream_ode_cases.solar_column_class and thermal_column_class), over the tables of the GPU
# tests at every depth, column count and order, the whole view and every observer.
# Where every level is clear the figure is the float64 rounding of the flux rows (the view
# mirrors read them as float64, as the kernels do).  Where every level is general it is the
# long-double mirror's own rounding, amplified as the mirrors' E_CPU notes describe: P and Q are
# divided by n = 1 - (Gamma*E)^2, about 1e-5 just above the conservative threshold (the spectral
# case has such levels: 3.78e-15; the grey general tables give 9.3e-17), and with the linear source
# u1 and d0 carry the shift c, 1e2 of pi*dB in a level of t = 9e-3 (2.04e-15, in the level t =
# 9.1e-3, w = 1 - 1.3e-6 of the 64 x 2 table; with the float64 rounding of the rows removed by
# linearity the isothermal grey figure falls to 1.8e-17 and this one stays).  The shortwave
# general figure is two_stream_ode_cases.SOLAR_TABLES' (3.3e-15) passed on.
CHAIN = {"isothermal": {"clear": 7.2e-17,           # measured 7.16e-17
                        "general": 3.8e-15,         # measured 3.783e-15
                        "conservative": 2.19e-9},   # measured 2.1832e-9
         "linear": {"clear": 7.4e-17,               # measured 7.35e-17
                    "general": 2.1e-15,             # measured 2.040e-15
                    "conservative": 1.83e-9},       # measured 1.8294e-9
         "solar": {"general": 5.4e-15,              # measured 5.35e-15
                   "conservative": 8.4e-11,         # measured 8.32e-11
                   "guarded": 9.62e-6}}             # measured 9.6107e-6
# The largest |change of the long-double view mirror|/scale per unit |change of one flux row|/(flux
# scale), over the same tables (the longwave whole view and every observer in both directions, the
# shortwave whole view): a row moved by 2^-10 of pi*scale or of F0.  It is 1 to rounding: the
# surface line of a path with eps = 0 or A = 1 hands down[L] over as it is.
GAIN = {"isothermal": 1.01,         # measured 1.0000000000001
        "linear": 1.01,             # measured 1.0000000000001
        "solar": 1.01}              # measured 1.0000000000001


# ---------------------------------------------------------------------------------------------
# A layer as an operator of the fluxes and of the two rays.
class View(object):
    """flux: two_stream_ode_cases' Operator.  The upward ray leaves the top: ul what the layer
    takes out of it (ut = 1 - ul is its transmittance), u_dn and u_up what a unit of I- entering
    the top and of I+ entering the bottom add to it, u_src [sources, ...] what each unit source
    adds.  The downward ray leaves the bottom: dl (dt = 1 - dl), d_dn, d_up and d_src, the same.

    As in the Operator what is lost is carried, not what is transmitted: a sublayer takes far less
    out of a ray than 1, a layer is made of up to 2^26 of them, and a product of that many
    transmittances would keep that many roundings of 1."""
    NAMES = ("ul", "u_dn", "u_up", "u_src", "dl", "d_dn", "d_up", "d_src")

    def __init__(self, flux, *parts):
        self.flux = flux
        for name, value in zip(self.NAMES, parts):
            setattr(self, name, value)
        self.ut, self.dt = LD(1.) - self.ul, LD(1.) - self.dl

    def parts(self):
        return tuple(getattr(self, name) for name in self.NAMES)

    def where(self, mask, other):
        return View(self.flux.where(mask, other.flux),
                    *(np.where(mask, a, b) for a, b in zip(self.parts(), other.parts())))

    def lowered(self, lower, thickness):
        """The same layer `thickness` further from space: its sources as lower() moves them."""
        f = self.flux
        return View(ode.Operator(f.rt, f.rb, f.at, f.ab, lower(f.up, thickness),
                                 lower(f.dn, thickness)),
                    self.ul, self.u_dn, self.u_up, lower(self.u_src, thickness),
                    self.dl, self.d_dn, self.d_up, lower(self.d_src, thickness))


def star(a, b):
    """a (nearer space) on top of b.  The fluxes between the two, per unit of I- entering the top,
    of I+ entering the bottom and of every source, are two_stream_ode_cases.star's; each ray
    passes one layer, collects what that layer makes of them, and passes the other."""
    fa, fb = a.flux, b.flux
    one = LD(1.)
    m = one/(one - fa.rb*fb.rt)
    dn_t, dn_b, dn_s = fa.td*m, fa.rb*(fb.tu*m), (fa.dn + fa.rb*fb.up)*m
    up_t, up_b, up_s = fb.rt*(fa.td*m), fb.tu*m, (fb.up + fb.rt*fa.dn)*m
    return View(ode.star(fa, fb),
                a.ul + a.ut*b.ul,
                a.u_dn + a.u_up*up_t + a.ut*(b.u_dn*dn_t),
                a.u_up*up_b + a.ut*(b.u_up + b.u_dn*dn_b),
                a.u_src + a.u_up*up_s + a.ut*(b.u_src + b.u_dn*dn_s),
                b.dl + b.dt*a.dl,
                b.d_dn*dn_t + b.dt*(a.d_dn + a.d_up*up_t),
                b.d_up + b.d_dn*dn_b + b.dt*(a.d_up*up_b),
                b.d_src + b.d_dn*dn_s + b.dt*(a.d_src + a.d_up*up_s))


def sublayer(matrix, h, dif, sources):
    """The View of a sublayer so thin that the power series of p = exp(M h) is exact to rounding.
    The states are (I+, I-, the source states, U, D): U = pi*I of the upward ray and D of the
    downward one are the last two.  With y(h) = p y(0) and I+(0) = rt I-(0) + tu I+(h) + up s,
        U(0) = (U(h) - p[U,0] I+(0) - p[U,1] I-(0) - p[U,s] s)/p[U,U]
        D(h) = p[D,D] D(0) + p[D,0] I+(0) + p[D,1] I-(0) + p[D,s] s
    (p[U,0], p[U,1] and p[U,s] are negative: every term adds)."""
    one = LD(1.)
    flux = ode.sublayer(matrix, h, dif, sources)
    a = matrix*h[..., None, None]
    e = np.matmul(a, ode.integral(a))                               # p - 1
    u, d = matrix.shape[-1] - 2, matrix.shape[-1] - 1
    ut = one/(one + e[..., u, u])
    return View(flux,
                e[..., u, u]*ut, -(e[..., u, 0]*flux.rt + e[..., u, 1])*ut, -(e[..., u, 0]*flux.tu)*ut,
                np.stack([-(e[..., u, 0]*flux.up[i] + e[..., u, 2 + i])*ut
                          for i in range(sources)]),
                -e[..., d, d], e[..., d, 0]*flux.rt + e[..., d, 1], e[..., d, 0]*flux.tu,
                np.stack([e[..., d, 0]*flux.up[i] + e[..., d, 2 + i] for i in range(sources)]))


def doubled(matrix, t, dif, sources, lower):
    """two_stream_ode_cases.doubled for a View; lower(vector [sources, ...], H): what the unit
    sources of a layer send anywhere as the layer lies H further from space."""
    with np.errstate(all="ignore"):
        norm = np.max(np.sum(np.abs(matrix), axis=-1), axis=-1)
        size = (norm*t*LD(ode.SERIES_NORM)).astype(F64)
        n = np.where(size > 1., np.ceil(np.log2(np.where(size > 1., size, 1.))), 0.).astype(int)
        h = t/LD(2.)**n
        op = sublayer(matrix, h, dif, sources)
        for j in range(int(np.max(n, initial=0))):
            op = star(op, op.lowered(lower, h*LD(2.)**j)).where(j < n, op)
    return op


def _ray_rows(m, mu, w, a, source_columns, source):
    """The rows of U and D: pi*J+- = (w/2)*[I_with*(1 + a) + I_against*(1 - a)] + source*(the
    states source_columns)."""
    one, two = LD(1.), LD(2.)
    u, d = m.shape[-1] - 2, m.shape[-1] - 1
    forth, back = (w/two)*(one + a)/mu, (w/two)*(one - a)/mu
    m[..., u, u], m[..., u, 0], m[..., u, 1] = one/mu, -forth, -back
    m[..., d, d], m[..., d, 0], m[..., d, 1] = -one/mu, back, forth
    for column in source_columns:
        m[..., u, column], m[..., d, column] = -source/mu, source/mu


def thermal_view(li, mu):
    """The View of every level from thermal_cases.layer_inputs' float64 t, w, gp and D and the
    view cosine mu (broadcastable to the elements): the sources are pi*B = 1 and pi*B = tau."""
    t, w, gp = (np.asarray(li[name], dtype=F64).astype(LD) for name in ("t", "w", "gp"))
    d = LD(li["d"])
    mu = np.broadcast_to(np.asarray(mu, dtype=F64), t.shape).astype(LD)
    one, two, three = LD(1.), LD(2.), LD(3.)
    g2 = d*w*(one - gp)/two
    dif = d*(one - w)
    g1 = g2 + dif
    # States: I+, I-, c (pi*B = c), u (tau' = u), tau (pi*B = tau), U, D.
    m = np.zeros(t.shape + (7, 7), dtype=LD)
    m[..., 0, 0], m[..., 0, 1], m[..., 0, 2], m[..., 0, 4] = g1, -g2, -dif, -dif
    m[..., 1, 0], m[..., 1, 1], m[..., 1, 2], m[..., 1, 4] = g2, -g1, dif, dif
    m[..., 4, 3] = one
    _ray_rows(m, mu, w, three*gp*mu/two, (2, 4), one - w)

    def lower(vector, thickness):
        # pi*B = tau of the whole is thickness + tau of the lower half.
        return np.stack([vector[0], thickness*vector[0] + vector[1]])
    return doubled(m, t, dif, 2, lower), t


def phase(vi, cos_theta):
    """Pmix in long double from view_inputs' float64 tau_R, w_c, tau_s, gc and cosT (0 where
    nothing scatters: there omega/sc is 0 too)."""
    one, two, three, four = LD(1.), LD(2.), LD(3.), LD(4.)
    tau_r, w_c, tau_s, gc = (np.asarray(vi[name], dtype=F64).astype(LD)
                             for name in ("tau_r", "w_c", "tau_s", "gc"))
    c = np.asarray(cos_theta, dtype=F64).astype(LD)
    with np.errstate(all="ignore"):
        pr = three*(one + c*c)/four
        ph = (one - gc*gc)/((one + gc*gc) - two*gc*c)**(three/two)
        dark = tau_s == 0.
        return np.where(dark, 0., (tau_r*pr + w_c*ph)/np.where(dark, one, tau_s))


def solar_view(vi, mu, cos_theta):
    """The View of every level from solar_radiance_cases.view_inputs' float64 t, w, gp, mu0,
    omega/sc and the phase function's inputs, the view cosine mu and cosT (broadcastable): the
    source is the beam, 1 at the top of the level."""
    empty = np.asarray(vi["tau"]) == 0.
    t, w, gp, mu0, osc = (np.where(empty & (name != "mu0"), 0., np.asarray(vi[name], dtype=F64))
                          .astype(LD) for name in ("t", "w", "gp", "mu0", "osc"))
    mu = np.broadcast_to(np.asarray(mu, dtype=F64), t.shape).astype(LD)
    one, two, three, four = LD(1.), LD(2.), LD(3.), LD(4.)
    g2 = three*w*(one - gp)/four
    g1 = g2 + two*(one - w)
    g3 = (two - three*mu0*gp)/four
    g4 = one - g3
    # States: I+, I-, s, U, D.
    m = np.zeros(t.shape + (5, 5), dtype=LD)
    m[..., 0, 0], m[..., 0, 1], m[..., 0, 2] = g1, -g2, -(w*g3)/mu0
    m[..., 1, 0], m[..., 1, 1], m[..., 1, 2] = g2, -g1, (w*g4)/mu0
    m[..., 2, 2] = -one/mu0
    _ray_rows(m, mu, w, three*gp*mu/two, (2,), (osc*phase(vi, cos_theta)/four)/mu0)

    def lower(vector, thickness):
        return np.exp(-thickness/mu0)*vector
    return doubled(m, t, two*(one - w), 1, lower), t, mu0


# ---------------------------------------------------------------------------------------------
# A column: the interface fluxes of two_stream_ode_cases, and each ray through the levels.
def rays(view, up, down, source_up, source_down, start):
    """pi*I at the L + 1 interfaces [L + 1, ...] of the upward ray from `start` at the surface and
    of the downward ray from 0 at space: `view` of L levels [L, ...], the interface fluxes up and
    down [L + 1, ...] and what the sources of each level add to either ray [L, ...]."""
    levels = view.ut.shape[0]
    looking_down = np.zeros(up.shape, dtype=LD)
    looking_up = np.zeros(up.shape, dtype=LD)
    looking_down[levels] = start
    for i in range(levels - 1, -1, -1):
        looking_down[i] = view.ut[i]*looking_down[i + 1] + view.u_dn[i]*down[i] + \
            view.u_up[i]*up[i + 1] + source_up[i]
    for i in range(levels):
        looking_up[i + 1] = view.dt[i]*looking_up[i] + view.d_dn[i]*down[i] + \
            view.d_up[i]*up[i + 1] + source_down[i]
    return looking_down, looking_up


def thermal_reference(inputs, mu, from_last, li=None):
    """{linear: {"down", "up": the radiance at the L + 1 interfaces [L + 1, PATHS, columns] (0
    faces space) seen looking down and looking up, "scale" [PATHS, columns], "flux": the
    interface fluxes {"up", "down"} [L + 1, PATHS, columns]}} of a thermal_source_cases.Inputs
    (or a scatterer_cases.Longwave) under the view cosines mu [PATHS], from the equations."""
    if li is None:
        li = inputs.layer_inputs(from_last)
    mu = np.asarray(mu, dtype=F64)
    view, t = thermal_view(li, mu[None, :, None])
    f = view.flux
    safe = np.where(t > 0., t, LD(1.))

    def ramp(vector):
        return np.where(t > 0., vector/safe, 0.)
    layers = (f.rt, f.td, f.up[0], ramp(f.up[1]), ramp(f.dn[1]))
    order = inputs.order(from_last).T                               # [L, PATHS]
    eps = inputs.emissivity[:, None] if inputs.emissivity.ndim == 1 else inputs.emissivity
    eps = np.asarray(eps, dtype=F64).astype(LD)
    nu = inputs.nu[None, None, :]
    surface_b = tc.pi_planck(LD, inputs.nu[None, :], inputs.surface_t[:, None])
    pi = LD(cases.FLUX_PI)
    out = {}
    for linear in (False, True):
        if linear:
            space = 1 if from_last else 0
            edges = inputs.edges[order]                             # [L, PATHS, 2]
            bt = tc.pi_planck(LD, nu, edges[:, :, space, None])
            bb = tc.pi_planck(LD, nu, edges[:, :, 1 - space, None])
            scale = rsc.scale(inputs)
        else:
            bt = bb = tc.pi_planck(LD, nu, inputs.table[order][:, :, None, 4])
            scale = rc.scale(inputs)
        flux = ode.thermal_column(layers, bt, bb, eps, surface_b)
        db = bb - bt
        start = eps*surface_b + (LD(1.) - eps)*flux["down"][-1]
        down, up = rays(view, flux["up"], flux["down"], bt*view.u_src[0] + db*ramp(view.u_src[1]),
                        bt*view.d_src[0] + db*ramp(view.d_src[1]), start)
        out[linear] = {"down": down/pi, "up": up/pi, "scale": scale, "flux": flux}
    return out


def solar_reference(inputs, mu, cos_theta, from_last, vi=None):
    """{"down": the radiance at the L + 1 interfaces [L + 1, PATHS, columns] seen looking down,
    "flux": {"up", "direct", "diffuse"} [L + 1, PATHS, columns]} of a two_stream_cases.Inputs (or
    a scatterer_cases.Shortwave: vi its view inputs) from the equations."""
    if vi is None:
        vi = svc.problem_inputs(inputs, from_last)
    mu = np.asarray(mu, dtype=F64)
    cos_theta = np.asarray(cos_theta, dtype=F64)
    view, t, mu0 = solar_view(vi, mu[None, :, None], cos_theta[None, :, None])
    f = view.flux
    with np.errstate(all="ignore"):
        layers = (f.rt, f.td, f.up[0], f.dn[0], np.exp(-t/mu0))
    albedo = inputs.albedo[:, None] if inputs.albedo.ndim == 1 else inputs.albedo
    flux = ode.solar_column(layers, albedo, LD(1.))
    albedo = np.asarray(albedo, dtype=F64).astype(LD)
    start = albedo*(flux["direct"][-1] + flux["diffuse"][-1])
    beam = flux["direct"][:-1]
    down, _ = rays(view, flux["up"], flux["diffuse"], beam*view.u_src[0], beam*view.d_src[0],
                   start)
    f0 = inputs.f0().astype(LD)
    return {"down": f0*down/LD(cases.FLUX_PI), "flux": {q: f0*flux[q] for q in flux}}


# ---------------------------------------------------------------------------------------------
# The long-double mirror chain: the flux mirror feeding the view mirror.
def rows(fluxes, names):
    """Flux rows as the entries hand them over: contiguous float64."""
    return {q: np.ascontiguousarray(fluxes[q], dtype=F64) for q in names}


def spectral(inputs):
    return hasattr(inputs, "knots")


def thermal_flux_mirror(inputs, from_last, linear):
    """The long-double flux mirror of the problem's flux entry: {"up", "down"} [levels, columns]."""
    if linear:
        return tsc.mirror(LD, inputs, from_last)
    return tc.mirror(LD, inputs.isothermal(), from_last)


def thermal_problem(inputs, linear):
    """What the view mirrors take: the problem itself with the linear source, its isothermal()
    otherwise."""
    return inputs if linear else inputs.isothermal()


def thermal_view_mirror(inputs, mu, from_last, linear, passed, up, fluxes):
    """The long-double view mirror on the flux rows `fluxes`: the observer's, which with passed =
    L looking down is the whole view's (asserted in thermal_chain)."""
    return oc.mirror(LD, thermal_problem(inputs, linear), mu, from_last, passed, up,
                     fluxes)["radiance"]


def whole_view_mirror(inputs, mu, from_last, linear, fluxes):
    """The long-double mirror of the whole-view entry of the problem."""
    if linear:
        return rsc.mirror(LD, inputs, mu, from_last, fluxes)["radiance"]
    if spectral(inputs):
        return spectral_view.thermal_mirror(LD, inputs, mu, from_last, fluxes)["radiance"]
    return rc.mirror(LD, inputs.isothermal(), mu, from_last, fluxes)["radiance"]


def solar_flux_mirror(inputs, from_last):
    return ts.mirror(LD, inputs, from_last)


def solar_view_inputs(inputs, from_last):
    if spectral(inputs):
        return spectral_view.solar_view_inputs(inputs, from_last)
    return svc.problem_inputs(inputs, from_last)


def solar_view_mirror(inputs, mu, cos_theta, from_last, fluxes):
    """The long-double view mirror's dict ("radiance", "peak") on the flux rows `fluxes`."""
    if spectral(inputs):
        return spectral_view.solar_mirror(LD, inputs, mu, cos_theta, from_last, fluxes)
    return svc.mirror(LD, inputs, mu, cos_theta, from_last, fluxes)


def thermal_mirror_sweeps(problem, mu, from_last, fluxes):
    """{up: [L + 1, PATHS, columns]} of the long-double view mirror at every interface in one
    sweep -- thermal_radiance_observer_cases' own start line and level function, called as its
    mirror calls them: looking down the entry i is the observer after L - i levels, looking up
    after i."""
    order = problem.order(from_last)
    li = problem.layer_inputs(from_last)
    depth = problem.levels_per_path
    mu = np.asarray(mu, dtype=F64)
    out = {}
    for up in (False, True):
        field = np.zeros((depth + 1, PATHS, problem.columns), dtype=LD)
        if not up:
            field[depth] = oc.surface_line(LD, problem, from_last, fluxes)
        for step in range(depth):
            i = step if up else depth - 1 - step
            field[i + 1 if up else i] = oc.through(LD, problem, li, order, from_last, mu, i, up,
                                                   fluxes, field[i if up else i + 1])
        out[up] = field
    return out


# ---------------------------------------------------------------------------------------------
# The views of the GPU tests.
def observers(depth):
    """n_p in {0, 1, L - 1, L}, duplicates dropped."""
    return sorted({0, min(1, depth), max(depth - 1, 0), depth})


def passed(n):
    return np.full(PATHS, n, dtype=np.int32)


def cos_theta(inputs):
    """One phi of PHI per path, through solar_radiance_cases.scattering_cosine."""
    return svc.scattering_cosine(MU, inputs.mu0, PHI)


def at_observer(field, n, up):
    """[PATHS, columns] of a reference field [L + 1, PATHS, columns]: looking down the result is
    at interface L - n_p, looking up at n_p."""
    return field[n] if up else field[field.shape[0] - 1 - n]


THERMAL_MAKERS = {"general": ode.thermal_general, "conservative": ode.thermal_conservative}
SOLAR_MAKERS = {"general": ode.solar_general, "conservative": ode.solar_conservative,
                "guard": ode.solar_guard}


@functools.lru_cache(maxsize=None)
def thermal_case(name, columns, depth, from_last):
    """(inputs, thermal_reference's dict) of a table of two_stream_ode_cases ("spectral": its
    spectral longwave case), formed once."""
    inputs = ode.spectral_longwave() if name == "spectral" else THERMAL_MAKERS[name](columns, depth)
    return inputs, thermal_reference(inputs, MU, from_last)


@functools.lru_cache(maxsize=None)
def solar_case(name, columns, depth, from_last):
    """(inputs, cosT, solar_reference's dict) of a table of two_stream_ode_cases."""
    inputs = ode.spectral_shortwave() if name == "spectral" else SOLAR_MAKERS[name](columns, depth)
    cosine = cos_theta(inputs)
    return inputs, cosine, solar_reference(inputs, MU, cosine, from_last,
                                           solar_view_inputs(inputs, from_last))
