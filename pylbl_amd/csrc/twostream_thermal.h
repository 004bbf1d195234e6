// Two-stream longwave fluxes through clouds (Spectroscopy.compute_thermal_flux,
// lbl_path_thermal_two_stream; with kLinear Spectroscopy.compute_thermal_flux_linear,
// lbl_path_thermal_two_stream_source): upward and downward fluxes at every interface of whole
// paths, from a delta-scaled two-stream layer solution with a thermal source and the adding
// recurrences, over the "total" absorption block in HBM.  The source is the Planck function of the
// level temperature or, with kLinear, linear in the layer's (scaled) optical depth between its
// two faces.  The TU builds with -ffp-contract=off: every product, sum and quotient below is
// rounded as written.
//
// Per level l the table row is (s_l, tau_c, w_c, g_c, T_l); D is the diffusivity factor, one
// scalar per call; piB(T) = kFluxPi*planck(nu, c1nu3, c2nu, T) (radiance.h, flux.h).
//   tau_a = s_l*beta ; tau = tau_a + tau_c
//   clear level (w_c == 0, the same for the whole wavefront):
//     x = D*tau ; R = 0 ; T = exp(-x) ; em = -expm1(-x)
//   cloudy level (w_c > 0; f = g_c*g_c and gp = g_c/(1 + g_c) are level scalars):
//     omega = w_c/tau ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc
//     g2 = (D*(w*(1 - gp)))/2 ; dif = D*(1 - w) ; g1 = g2 + dif ; su = g1 + g2 ; k2 = dif*su
//     conservative, where k2*(1 + t*t) <= 1e-10:
//       x = g1*t ; R = x/(1 + x) ; T = 1/(1 + x) ; em = (dif*t)/(1 + x)
//     general:
//       k = sqrt(k2) ; E = exp(-(k*t)) ; E2 = E*E ; o1 = -expm1(-(2*(k*t)))
//       den = k*(1 + E2) + g1*o1 ; R = (g2*o1)/den ; T = (2*(k*E))/den
//       em = (k*((1 - E)*(1 - E)) + dif*o1)/den        (= 1 - R - T, without the cancellation)
//   S = piB(T_l)*em        the layer's own emission, the same upward and downward
// Adding, interface 0 facing space, level i between interfaces i and i + 1 in the order space ->
// surface, eps the surface emissivity and T_s its temperature:
//   up, from the surface:  Rs[L] = 1 - eps ; U[L] = eps*piB(T_s) ;  for i = L-1 .. 0:
//     m1 = 1/(1 - R_i*Rs[i+1])
//     U[i] = S_i + T_i*((U[i+1] + Rs[i+1]*S_i)*m1)
//     Rs[i] = R_i + T_i*((T_i*Rs[i+1])*m1)
//   down, from space:  Dn = 0, Rd = 0 ;  at every interface i = 0 .. L:
//     m2 = 1/(1 - Rd*Rs[i])
//     down[i] = (Dn + Rd*U[i])*m2 ; up[i] = (U[i] + Rs[i]*Dn)*m2
//     then through level i:  m3 = 1/(1 - Rd*R_i)
//     Dn = S_i + T_i*((Dn + Rd*S_i)*m3) ; Rd = R_i + T_i*((T_i*Rd)*m3)
// A clear level has R = 0, so m1 = m3 = 1 exactly, x*1 = x and 0 + x = x: thermal_through leaves
// those out where the level is clear and gives the bits of the lines above.
//
//
// kLinear: the table row, D, tau, t, w, g1, g2, dif, su, k2, k, E, E2, o1, den, R, T, em, x and the
// branch conditions are the ones above, bit for bit; T_l is not read.  Per level and column,
// Bt = piB(T at the level's space-side interface), Bb = piB(T at its surface-side interface),
// dB = Bb - Bt, and the layer sends
//   S_up = Bt*em + dB*q        out of its space-side face
//   S_dn = Bb*em - dB*q        out of its surface-side face
// q = (1 - T + R)/(su*t) - T from the particular solution F+- = pi*(B(tau) +- B'/su), formed
// without the difference, which cancels to O(t) in a thin layer:
//   clear level (w_c == 0):  q = a - linear_weight(x, a)
//     (a = em = -expm1(-x); radiance.h's linear_weight: the u_in of lbl_path_flux_source)
//   cloudy, general:  y = k*t ; z = y*y
//     p = o1 - 2*(y*E)                                        for y >= 1/2
//     p = E*(((y*z)/3)*(1 + z*(1/20 + z*(1/840 + z*(1/60480 + z*(1/6652800 + z*(1/1037836800
//         + z*(1/217945728000 + z*(1/59281238016000)))))))))    for y < 1/2
//       (p = 2*E*(sinh y - y) = 1 - E2 - 2*y*E; the direct form loses y's leading digits)
//     q = ((k*(o1*o1))/(su*((1 + E)*(1 + E))) + p)/(den*t)
//       (o1/(1 + E) is 1 - E without its cancellation: em's (1 - E)*(1 - E) loses y's leading
//       digits, which em does not feel beside dif*o1 and q does, 1.4e-8 relative at y = 1e-8)
//   cloudy, conservative:  q = ((dif*t)*(1 + (su*t)/3))/(2*(1 + x))
// With dB = 0 both sources are Bt*em exactly: a path whose interface and level temperatures are
// all equal has the bits of the source above.  Adding is the one above with the two sources told
// apart:
//   up:    U[i] = S_up_i + T_i*((U[i+1] + Rs[i+1]*S_dn_i)*m1)
//   down:  Dn   = S_dn_i + T_i*((Dn + Rd*S_up_i)*m3)
// Rs, Rd, m1, m2, m3, the interface lines and the surface (eps*piB(T_s), 1 - eps) are unchanged:
// T_s is not the interface temperature at the surface.
//
// thermal_layer is the layer written once, with q where kLinear; ThermalFaces::through, the step
// through one level, calls it for both sweeps and both sources.  w_c == 0 is a wave-uniform branch
// (the level's scalars are the same for the whole wavefront): a clear level costs one exp, one
// expm1 and the Planck function, no square root and no division of the layer or the adding (with
// kLinear: one division, linear_weight's).  The kernels run on path.h's sweep skeleton, whole paths
// only, as twostream.h's do: thermal_up_kernel sweeps surface -> space with U and Rs in registers
// and writes them to the work rows at the interface above each level; thermal_down_kernel, queued
// behind it on the same stream, sweeps space -> surface with Dn and Rd in registers, reads beta
// again and recomputes the layer instead of reading three stored quantities (48 B per element
// beside beta's 8 B), reads the work rows and stores the flux rows asked for; the lane that starts
// a path writes the rows of interface 0.  nu, C2*nu and C1*nu^3 are formed once per lane, as in
// flux.h.  With kLinear, as in radiance.h's kLinear sweeps, a lane evaluates Planck once at the
// face it enters its path through and then once per level at the exit face, which it keeps as the
// next level's entry value (the table is continuous within a path: the entry checks it): one
// Planck per element and level, as without.
//
// kSpectral (lbl_path_thermal_two_stream_spectral, either source): tau_c, w_c and g_c of a level
// come per grid point from the scatterer's knot table (scatterer.h) in place of the level row: a
// lane finds where its columns lie among the knots once, before its sweep; per level and column
// it fills the ThermalLevel the one thermal_layer takes -- tau_c interpolated and limited, and in a
// level that scatters w_c = omega_c*tau_c, f = g_c*g_c and gp = g_c/(1 + g_c) of the column.
// Whether a level scatters (some knot has omega_c*tau_c != 0) is one word per level from the
// host: a level that does not stays clear for the whole wavefront, with its tau_c(nu).  In a level
// that scatters an element whose tau = s_l*beta + tau_c is 0 takes the clear branch (x = 0: the
// identity), where the cloudy one would form 0/0 -- a grey cloudy level has tau >= tau_c > 0.
// Without kSpectral nothing of this is read or compiled.  Going up with the level-temperature
// source the spectral kernel keeps two rows in flight (kThermalSpectralUpAhead): four and eight
// spill scalar registers.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/lbl_amd.h"
#include "flux.h"
#include "path.h"
#include "radiance.h"
#include "scatterer.h"

namespace lbl {

constexpr double kThermalConservative = 1e-10;      // k2*(1 + t*t) at most: the conservative branch
constexpr int kThermalLevelWords = 5;               // s_l, tau_c, w_c, g_c, T_l per level
constexpr int kThermalUpAhead = kPathAhead;         // rows of beta in flight per lane, going up
constexpr int kThermalDownAhead = 1;              // going down: more rows spill scalar registers
constexpr double kThermalSourceSeriesBelow = 1./2.; // y = k*t below which p comes from its series
constexpr int kThermalSourceUpAhead = 1;            // kLinear, going up: more rows spill scalar registers
constexpr int kThermalSourceDownAhead = 1;          // going down
constexpr int kThermalSpectralUpAhead = 2;          // kSpectral, going up: 4 spill scalar registers
static_assert(kThermalSourceDownAhead == kThermalDownAhead, "the down kernel takes one for both");

struct PathThermal : PathLevels
{
    const double * nu;          // [columns]: the grid [cm-1]
    const double * level;       // [count][5]: s_l, tau_c, w_c, g_c, T_l of flat level first + i
    double diffusivity;         // D
    const double * surface_t;   // [paths of the run]: surface temperature [K]
    const double * surface_e;   // [paths of the run]: scalar emissivity (without emissivity_rows)
    int table_path;             // path of surface_t[0] / surface_e[0]
    const double * emissivity_rows; // [paths][stride]: eps per path and column, or null
    double * work;              // [count][2][stride]: U, Rs at the interface above each level
    double * level_out[2];      // up, down at the interface below each level (null: not wanted)
    double * top_out[2];        // [paths][stride]: the same at interface 0
    const double * edge;        // kLinear: [count][2], interface temperatures of flat level
                                // first + i on its first-level / last-level side [K]; else null
};

// lbl_path_thermal_two_stream_spectral's: the same with the scatterer's knot table, which replaces
// tau_c, w_c and g_c of the level rows (0 there) per grid point.
struct PathThermalSpectral : PathThermal
{
    ScattererKnots scatterer;
    const double * scatters;    // [count]: 0 where every knot of flat level first + i has
                                // omega_c*tau_c == 0 (a clear level), else 1
};

template <bool kSpectral>
using ThermalArguments = std::conditional_t<kSpectral, PathThermalSpectral, PathThermal>;

// What a layer does to diffuse light, the fraction of piB(T_l) it emits either way and, with
// kLinear, the weight q of the Planck difference across it.
struct ThermalLayer
{
    double r, t, em, q;
};

// The level's scalars, read once per level and wavefront.
struct ThermalLevel
{
    double s, tau_c, w_c, f, gp, temperature;
    bool clear;
};

__device__ __forceinline__ ThermalLevel thermal_level(const double * row)
{
    ThermalLevel v;
    v.s = row[0];
    v.tau_c = row[1];
    v.w_c = row[2];
    v.temperature = row[4];
    v.clear = v.w_c == 0.;
    v.f = 0.;
    v.gp = 0.;
    if (!v.clear)
    {
        const double g_c = row[3];
        v.f = g_c*g_c;
        v.gp = g_c/(1. + g_c);
    }
    return v;
}

// p = 2*E*(sinh y - y) for y = k*t >= 0, E = exp(-y) and o1 = 1 - E*E.
__device__ __forceinline__ double thermal_source_p(double y, double e, double o1)
{
    const double z = y*y;
    const double series =
        1. + z*(1./20. + z*(1./840. + z*(1./60480. + z*(1./6652800. + z*(1./1037836800. +
        z*(1./217945728000. + z*(1./59281238016000.)))))));
    return y < kThermalSourceSeriesBelow ? e*(((y*z)/3.)*series) : o1 - 2.*(y*e);
}

// The layer of one level and grid point (the formulas in the head of this file).  v: the level's
// scalars; d: the diffusivity factor; b: beta.
template <bool kLinear>
__device__ __forceinline__ ThermalLayer thermal_layer(const ThermalLevel & v, double d, double b)
{
    ThermalLayer y;
    const double tau_a = v.s*b;
    const double tau = tau_a + v.tau_c;
    if (v.clear)
    {
        const double x = d*tau;
        y.r = 0.;
        y.t = exp(-x);
        y.em = -expm1(-x);
        if constexpr (kLinear) y.q = y.em - linear_weight(x, y.em);
        return y;
    }
    const double omega = v.w_c/tau;
    const double sc = 1. - omega*v.f;
    const double t = sc*tau;
    const double w = ((1. - v.f)*omega)/sc;
    const double g2 = (d*(w*(1. - v.gp)))/2.;
    const double dif = d*(1. - w);
    const double g1 = g2 + dif;
    const double su = g1 + g2;
    const double k2 = dif*su;
    if (k2*(1. + t*t) <= kThermalConservative)
    {
        const double x = g1*t;
        y.r = x/(1. + x);
        y.t = 1./(1. + x);
        y.em = (dif*t)/(1. + x);
        if constexpr (kLinear) y.q = ((dif*t)*(1. + (su*t)/3.))/(2.*(1. + x));
        return y;
    }
    const double k = sqrt(k2);
    const double e = exp(-(k*t));
    const double e2 = e*e;
    const double o1 = -expm1(-(2.*(k*t)));
    const double den = k*(1. + e2) + g1*o1;
    y.r = (g2*o1)/den;
    y.t = (2.*(k*e))/den;
    y.em = (k*((1. - e)*(1. - e)) + dif*o1)/den;
    if constexpr (kLinear)
    {
        y.q = ((k*(o1*o1))/(su*((1. + e)*(1. + e))) + thermal_source_p(k*t, e, o1))/(den*t);
    }
    return y;
}

// One adding step through a level, the same lines upward and downward: what arrives (flux, with
// the reflectance refl of what lies behind it) becomes what leaves on the level's other side.
// `out` is the layer's source through the face the sweep leaves the level by, `back` through the
// one it entered by (the level-temperature source: the same S twice).
//   m = 1/(1 - R*refl) ; flux = out + T*((flux + refl*back)*m) ; refl = R + T*((T*refl)*m)
// clear: R = 0 and m = 1 exactly, left out.
__device__ __forceinline__ void thermal_through(bool clear, const ThermalLayer & y, double out,
                                                double back, double & flux, double & refl)
{
    if (clear)
    {
        flux = out + y.t*(flux + refl*back);
        refl = y.t*(y.t*refl);
        return;
    }
    const double m = 1./(1. - y.r*refl);
    flux = out + y.t*((flux + refl*back)*m);
    refl = y.r + y.t*((y.t*refl)*m);
}

// What a lane forms once of its columns of the grid.
struct ThermalColumns
{
    double nu[kPathWidth], c1nu3[kPathWidth], c2nu[kPathWidth];
};

template <bool kVector>
__device__ __forceinline__ ThermalColumns thermal_columns(const PathThermal & a, const PathLane & l)
{
    ThermalColumns c;
    path_load<kVector>(a.nu + l.j, l.width, c.nu);
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        c.c1nu3[i] = ((LBL_PLANCK_C1*c.nu[i])*c.nu[i])*c.nu[i];
        c.c2nu[i] = LBL_PLANCK_C2*c.nu[i];
    }
    return c;
}

__device__ __forceinline__ double thermal_pi_planck(const ThermalColumns & c, int i, double t)
{
    return kFluxPi*planck(c.nu[i], c.c1nu3[i], c.c2nu[i], t);
}

// The surface of path l.p: U[L] = eps*piB(T_s) and Rs[L] = 1 - eps.
template <bool kVector>
__device__ __forceinline__ void thermal_surface(const PathThermal & a, const PathLane & l,
                                                const ThermalColumns & c, double (&u)[kPathWidth],
                                                double (&rs)[kPathWidth])
{
    double eps[kPathWidth];
    if (a.emissivity_rows != nullptr)
    {
        path_load<kVector>(a.emissivity_rows + (long long)l.p*a.stride + l.j, l.width, eps);
    }
    else
    {
        const double scalar = a.surface_e[l.p - a.table_path];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) eps[i] = scalar;
    }
    const double ts = a.surface_t[l.p - a.table_path];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        rs[i] = 1. - eps[i];
        u[i] = eps[i]*thermal_pi_planck(c, i, ts);
    }
}

// The two fluxes of an interface where what comes from above is (dn, rd) and what lies below
// sends up u and reflects rs, stored at offset `at` of the rows `out` (null: not wanted).
template <bool kVector>
__device__ __forceinline__ void thermal_interface(
    double * const (&out)[2], long long at, int width, const double (&dn)[kPathWidth],
    const double (&rd)[kPathWidth], const double (&u)[kPathWidth], const double (&rs)[kPathWidth])
{
    double up[kPathWidth], down[kPathWidth];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        const double m2 = 1./(1. - rd[i]*rs[i]);
        down[i] = (dn[i] + rd[i]*u[i])*m2;
        up[i] = (u[i] + rs[i]*dn[i])*m2;
    }
    if (out[0] != nullptr) path_store<kVector>(out[0] + at, width, up);
    if (out[1] != nullptr) path_store<kVector>(out[1] + at, width, down);
}

// The step of a sweep through one level, for both sweeps and both sources, and what a lane
// carries from level to level for it: with kLinear piB at the face it enters the next level by.
template <bool kLinear, bool kSpectral = false>
struct ThermalFaces
{
    const double * level;       // the table rows, at the lane's first level
    const double * edge;        // kLinear: the interface temperatures, likewise
    int side;                   // kLinear: which of a level's two it is entered by
    double d;
    double entry[kPathWidth];
    ScattererKnots scatterer;   // kSpectral: the knot table, its rows at the lane's first level,
    const double * scatters;    // whether a level scatters, likewise, and where the lane's
    ScattererLane knots;        // columns lie among the knots

    __device__ __forceinline__ ThermalFaces(const ThermalArguments<kSpectral> & a,
                                            const PathLane & l, const ThermalColumns & c)
        : level(a.level + (long long)l.index0*kThermalLevelWords), edge(nullptr), side(0),
          d(a.diffusivity)
    {
        if constexpr (kLinear)
        {
            side = entry_side(l.direction);
            edge = a.edge + 2*(long long)l.index0;
            const double t = edge[side];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i) entry[i] = thermal_pi_planck(c, i, t);
        }
        if constexpr (kSpectral)
        {
            scatterer = a.scatterer;
            scatterer.optics = scatterer_rows(a.scatterer, l.index0);
            scatters = a.scatters + l.index0;
            knots = scatterer_lane(a.scatterer, c.nu);
        }
    }

    // kSpectral: the scalars of level k of the sweep at the lane's column i with beta b, from the
    // level's three knot rows.  A level none of whose knots scatters stays clear for the whole
    // wavefront, with its absorption tau_c(nu); in a level that scatters every element takes the
    // cloudy branches with w_c = omega_c*tau_c, f = g_c*g_c and gp = g_c/(1 + g_c) of its own
    // column -- also one whose w_c is 0 --, but where tau = s*beta + tau_c is 0 the cloudy
    // branches would form 0/0 and the element takes the clear one: x = 0, the identity.
    __device__ __forceinline__ void element(const PathLane & l, int k, int i, double b,
                                            ThermalLevel & v) const
    {
        const int m = scatterer.n_knots;
        const double * rows = scatterer.optics + (long long)(k*l.direction)*(kScattererWords*m);
        v.tau_c = scatterer_value(rows, knots.j[i], knots.u[i]);
        if (v.clear) return;
        const double omega_c = scatterer_value(rows + m, knots.j[i], knots.u[i]);
        const double g_c = scatterer_value(rows + 2*m, knots.j[i], knots.u[i]);
        v.w_c = omega_c*v.tau_c;
        v.f = g_c*g_c;
        v.gp = g_c/(1. + g_c);
        v.clear = v.s*b + v.tau_c == 0.;
    }

    // Level k of the sweep with beta b: (flux, refl) on the side the lane came from become those
    // on the side it goes to.  The exit face has the level temperature or, with kLinear, its
    // interface's; there, with S_up and S_dn of the head in terms of the face the lane enters by
    // and the one it leaves by,
    //   db = entry - leave ; out = leave*em + db*q ; back = entry*em - db*q
    // Going up (entry Bb, leave Bt) that is the head's text.  Going down (entry Bt, leave Bb) db
    // is -dB, out = Bb*em + (-dB)*q and back = Bt*em - (-dB)*q, which are the head's
    // S_dn = Bb*em - dB*q and S_up = Bt*em + dB*q to the bit: -(a - b) == b - a,
    // (-d)*q == -(d*q) and x + (-p) == x - p are exact in IEEE arithmetic, signed zeros included.
    __device__ __forceinline__ void through(const PathLane & l, const ThermalColumns & c, int k,
                                            const double (&b)[kPathWidth],
                                            double (&flux)[kPathWidth], double (&refl)[kPathWidth])
    {
        ThermalLevel scalars = thermal_level(level + (long long)(k*l.direction)*kThermalLevelWords);
        if constexpr (kSpectral) scalars.clear = scatters[k*l.direction] == 0.;
        double t_leave = scalars.temperature;
        if constexpr (kLinear) t_leave = edge[2*(long long)(k*l.direction) + (1 - side)];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            ThermalLevel v = scalars;
            if constexpr (kSpectral) element(l, k, i, b[i], v);
            const ThermalLayer y = thermal_layer<kLinear>(v, d, b[i]);
            const double leave = thermal_pi_planck(c, i, t_leave);
            double out = leave*y.em, back = out;
            if constexpr (kLinear)
            {
                const double db = entry[i] - leave;
                out = leave*y.em + db*y.q;
                back = entry[i]*y.em - db*y.q;
                entry[i] = leave;
            }
            thermal_through(v.clear, y, out, back, flux[i], refl[i]);
        }
    }
};

// grid and kVector as for path_sweep_kernel; a.from_last is the order of this sweep, surface to
// space: a level is entered through its surface-side face (Bb) and left through the other (Bt).
// Whole paths: every lane starts and finishes its path.
template <bool kVector, bool kLinear, bool kSpectral = false>
__global__ __launch_bounds__(kPathThreads) void thermal_up_kernel(ThermalArguments<kSpectral> a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const int width = l.width;
    const ThermalColumns c = thermal_columns<kVector>(a, l);

    double u[kPathWidth], rs[kPathWidth];
    thermal_surface<kVector>(a, l, c, u, rs);

    ThermalFaces<kLinear, kSpectral> faces(a, l, c);
    constexpr int kAhead = kLinear ? kThermalSourceUpAhead : kThermalUpAhead;
    const auto step = [&](int k, const double (&b)[kPathWidth], long long at) {
        faces.through(l, c, k, b, u, rs);
        double * work = a.work + (2*at - l.j);
        path_store<kVector>(work, width, u);
        path_store<kVector>(work + a.stride, width, rs);
    };
    if constexpr (kSpectral)
    {
        constexpr int kRows = kLinear ? kThermalSourceUpAhead : kThermalSpectralUpAhead;
        path_levels<kRows, kVector>(a, l, step);
    }
    else
    {
        path_levels<kAhead, kVector>(a, l, step);
    }
}

// grid and kVector as for path_sweep_kernel; a.from_last is the order space to surface: a level is
// entered through its space-side face (Bt) and left through the other (Bb).
template <bool kVector, bool kLinear, bool kSpectral = false>
__global__ __launch_bounds__(kPathThreads) void thermal_down_kernel(ThermalArguments<kSpectral> a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const int width = l.width;
    const ThermalColumns c = thermal_columns<kVector>(a, l);

    double dn[kPathWidth], rd[kPathWidth], u[kPathWidth], rs[kPathWidth];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i) dn[i] = rd[i] = 0.;
    // Interface 0: what the whole path sends up and reflects is in the work rows of the first
    // level.
    {
        const double * work = a.work + (2*l.level0 - l.j);
        path_load<kVector>(work, width, u);
        path_load<kVector>(work + a.stride, width, rs);
        thermal_interface<kVector>(a.top_out, (long long)l.p*a.stride + l.j, width, dn, rd, u, rs);
    }
    ThermalFaces<kLinear, kSpectral> faces(a, l, c);
    path_levels<kThermalDownAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth],
                                                        long long at) {
        faces.through(l, c, k, b, dn, rd);
        // What lies below this level: the next level's work rows, or the surface.
        if (k + 1 < l.n)
        {
            const double * work = a.work + (2*(at + l.row_step) - l.j);
            path_load<kVector>(work, width, u);
            path_load<kVector>(work + a.stride, width, rs);
        }
        else
        {
            thermal_surface<kVector>(a, l, c, u, rs);
        }
        thermal_interface<kVector>(a.level_out, at, width, dn, rd, u, rs);
    });
}

}  // namespace lbl
