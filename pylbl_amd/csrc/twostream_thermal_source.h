// Two-stream longwave fluxes through clouds with a source that is linear in optical depth
// (Spectroscopy.compute_thermal_flux_linear, lbl_path_thermal_two_stream_source): twostream_thermal.h's
// layer and adding recurrences, with the Planck function varying linearly in the layer's (scaled)
// optical depth between its two faces instead of being that of the level temperature.  The TU
// builds with -ffp-contract=off: every product, sum and quotient below is rounded as written.
//
// Per level the table row (s_l, tau_c, w_c, g_c, T_l), D, tau, t, w, g1, g2, dif, su, k2, k, E, E2,
// o1, den, R, T, em, x and the branch conditions are twostream_thermal.h's, bit for bit; T_l is not
// read.  Per level and column, Bt = piB(T at the level's space-side interface), Bb = piB(T at its
// surface-side interface), dB = Bb - Bt, and the layer sends
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
// all equal has twostream_thermal.h's bits.
// Adding is twostream_thermal.h's with the two sources told apart:
//   up:    U[i] = S_up_i + T_i*((U[i+1] + Rs[i+1]*S_dn_i)*m1)
//   down:  Dn   = S_dn_i + T_i*((Dn + Rd*S_up_i)*m3)
// Rs, Rd, m1, m2, m3, the interface lines and the surface (eps*piB(T_s), 1 - eps) are unchanged:
// T_s is not the interface temperature at the surface.
//
// thermal_source_layer is the layer written once; both kernels call it.  w_c == 0 stays a
// wave-uniform branch.  The kernels run on path.h's sweep skeleton, whole paths only, and reuse
// thermal_level, thermal_columns, thermal_pi_planck, thermal_surface and thermal_interface.  As in
// radiance.h's kLinear sweeps a lane evaluates Planck once at the face it enters its path through
// and then once per level at the exit face, which it keeps as the next level's entry value (the
// table is continuous within a path: the entry checks it): one Planck per element and level.
#pragma once

#include <hip/hip_runtime.h>

#include "twostream_thermal.h"

namespace lbl {

constexpr double kThermalSourceSeriesBelow = 1./2.; // y = k*t below which p comes from its series
constexpr int kThermalSourceUpAhead = 1;            // going up: more rows spill scalar registers
constexpr int kThermalSourceDownAhead = 1;          // going down

struct PathThermalSource : PathThermal
{
    const double * edge;        // [count][2]: interface temperatures of flat level first + i on
                                // its first-level / last-level side [K]
};

// ThermalLayer with the weight q of the Planck difference across the layer.
struct ThermalSourceLayer
{
    double r, t, em, q;
};

// p = 2*E*(sinh y - y) for y = k*t >= 0, E = exp(-y) and o1 = 1 - E*E.
__device__ __forceinline__ double thermal_source_p(double y, double e, double o1)
{
    const double z = y*y;
    const double series =
        1. + z*(1./20. + z*(1./840. + z*(1./60480. + z*(1./6652800. + z*(1./1037836800. +
        z*(1./217945728000. + z*(1./59281238016000.)))))));
    return y < kThermalSourceSeriesBelow ? e*(((y*z)/3.)*series) : o1 - 2.*(y*e);
}

// The layer of one level and grid point (the formulas in the head of this file; r, t and em are
// thermal_layer's expressions, term for term).  v: the level's scalars; d: the diffusivity
// factor; b: beta.
__device__ __forceinline__ ThermalSourceLayer thermal_source_layer(const ThermalLevel & v,
                                                                   double d, double b)
{
    ThermalSourceLayer y;
    const double tau_a = v.s*b;
    const double tau = tau_a + v.tau_c;
    if (v.clear)
    {
        const double x = d*tau;
        y.r = 0.;
        y.t = exp(-x);
        y.em = -expm1(-x);
        y.q = y.em - linear_weight(x, y.em);
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
        y.q = ((dif*t)*(1. + (su*t)/3.))/(2.*(1. + x));
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
    y.q = ((k*(o1*o1))/(su*((1. + e)*(1. + e))) + thermal_source_p(k*t, e, o1))/(den*t);
    return y;
}

// thermal_through with the two sources of a layer: `out` leaves through the face the sweep leaves
// the level through, `back` through the one it entered.
//   m = 1/(1 - R*refl) ; flux = out + T*((flux + refl*back)*m) ; refl = R + T*((T*refl)*m)
// clear: R = 0 and m = 1 exactly, left out.
__device__ __forceinline__ void thermal_source_through(bool clear, const ThermalSourceLayer & y,
                                                       double out, double back, double & flux,
                                                       double & refl)
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

// grid and kVector as for path_sweep_kernel; a.from_last is the order of this sweep, surface to
// space: a level is entered through its surface-side face (Bb) and left through the other (Bt).
// Whole paths: every lane starts and finishes its path.
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void thermal_source_up_kernel(PathThermalSource a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const double * level = a.level + (long long)l.index0*kThermalLevelWords;
    const int width = l.width;
    const double d = a.diffusivity;
    const ThermalColumns c = thermal_columns<kVector>(a, l);

    double u[kPathWidth], rs[kPathWidth];
    thermal_surface<kVector>(a, l, c, u, rs);

    const int side = entry_side(l.direction);
    const double * edge = a.edge + 2*(long long)l.index0;
    double bb[kPathWidth];
    {
        const double t = edge[side];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) bb[i] = thermal_pi_planck(c, i, t);
    }
    path_levels<kThermalSourceUpAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth],
                                                            long long at) {
        const ThermalLevel v = thermal_level(level + (long long)(k*l.direction)*kThermalLevelWords);
        const double t_out = edge[2*(long long)(k*l.direction) + (1 - side)];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            const ThermalSourceLayer y = thermal_source_layer(v, d, b[i]);
            const double bt = thermal_pi_planck(c, i, t_out);
            const double db = bb[i] - bt;
            const double s_up = bt*y.em + db*y.q;
            const double s_dn = bb[i]*y.em - db*y.q;
            thermal_source_through(v.clear, y, s_up, s_dn, u[i], rs[i]);
            bb[i] = bt;
        }
        double * work = a.work + (2*at - l.j);
        path_store<kVector>(work, width, u);
        path_store<kVector>(work + a.stride, width, rs);
    });
}

// grid and kVector as for path_sweep_kernel; a.from_last is the order space to surface: a level is
// entered through its space-side face (Bt) and left through the other (Bb).
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void thermal_source_down_kernel(PathThermalSource a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const double * level = a.level + (long long)l.index0*kThermalLevelWords;
    const int width = l.width;
    const double d = a.diffusivity;
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
    const int side = entry_side(l.direction);
    const double * edge = a.edge + 2*(long long)l.index0;
    double bt[kPathWidth];
    {
        const double t = edge[side];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) bt[i] = thermal_pi_planck(c, i, t);
    }
    path_levels<kThermalSourceDownAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth],
                                                              long long at) {
        const ThermalLevel v = thermal_level(level + (long long)(k*l.direction)*kThermalLevelWords);
        const double t_out = edge[2*(long long)(k*l.direction) + (1 - side)];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            const ThermalSourceLayer y = thermal_source_layer(v, d, b[i]);
            const double bb = thermal_pi_planck(c, i, t_out);
            const double db = bb - bt[i];
            const double s_up = bt[i]*y.em + db*y.q;
            const double s_dn = bb*y.em - db*y.q;
            thermal_source_through(v.clear, y, s_dn, s_up, dn[i], rd[i]);
            bt[i] = bb;
        }
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
