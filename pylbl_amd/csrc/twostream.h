// Two-stream shortwave fluxes with scattering (Spectroscopy.compute_solar_flux, lbl_rayleigh_row,
// lbl_path_two_stream): upward, downward, direct and diffuse fluxes at every interface of whole
// paths, from a delta-scaled PIFM layer solution and the adding recurrences, over the "total"
// absorption block in HBM.  The TU builds with -ffp-contract=off: every product, sum and quotient
// below is rounded as written.
//
// Layer optics, per level l and grid point (s_l, c_l, tau_c, w_c, h_c: the level's table row):
//   tau_a = s_l*beta ;  tau_R = c_l*sigma(nu) ;  tau = (tau_a + tau_R) + tau_c
//   tau_s = tau_R + w_c ;  omega = tau_s/tau ;  g = h_c/tau_s  (g = 0 where tau_s == 0)
//   tau == 0: the layer is the identity (Rdif = Rdir = Tdp = 0, Tdif = D = 1)
// Delta scaling and PIFM coefficients (Zdunkowski):
//   f = g*g ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc ; gp = g/(1 + g)
//   g2 = (3*(w*(1 - gp)))/4 ; dif = 2*(1 - w) ; g1 = g2 + dif ; su = g1 + g2
//   g3 = (2 - 3*(mu0*gp))/4 ; g4 = 1 - g3 ; k2 = dif*su ; D = exp(-t/mu0)
// Conservative branch, where k2*(1 + t*t) <= kTwoStreamConservative:
//   x = g1*t ; Rdif = x/(1 + x) ; Tdif = 1/(1 + x)
//   Rdir = (x + (g3 - g1*mu0)*(-expm1(-t/mu0)))/(1 + x) ; Tdp = (1 - Rdir) - D
// General branch (Meador & Weaver 1980, scaled by exp(-k t)):
//   k = sqrt(k2) ; m = mu0 ; x = k*m
//   if |1 - x| < kTwoStreamResonance: m = (x >= 1 ? (1 + 1e-4) : (1 - 1e-4))/k ; x = k*m
//   Dm = exp(-t/m) ; E = exp(-(k*t)) ; E2 = E*E ; o1 = -expm1(-(2*(k*t)))
//   den = k*(1 + E2) + g1*o1 ; q = ((1 - x)*(1 + x))*den
//   Rdif = (g2*o1)/den ; Tdif = (2*(k*E))/den
//   a1 = g1*g4 + g2*g3 ; a2 = g1*g3 + g2*g4
//   Rdir = w*((1 - x)*(a2 + k*g3) - ((1 + x)*(a2 - k*g3))*E2 - (2*(k*(g3 - a2*m)))*(E*Dm))/q
//   Ttot = Dm*(1 - w*((1 + x)*(a1 + k*g4) - ((1 - x)*(a1 - k*g4))*E2)/q) + w*((2*(k*(g4 + a1*m)))*E)/q
//   Tdp = Ttot - Dm
// Adding, interface 0 facing space, level i between interfaces i and i + 1 in the Sun's order, A
// the albedo, F0 = mu0*S:
//   up:   Rup[L] = Rupd[L] = A ;  for i = L-1 .. 0:  m1 = 1/(1 - Rdif_i*Rupd[i+1])
//         Rup[i] = Rdir_i + Tdif_i*((Tdp_i*Rupd[i+1] + D_i*Rup[i+1])*m1)
//         Rupd[i] = Rdif_i + Tdif_i*((Tdif_i*Rupd[i+1])*m1)
//   down: Tb = 1, Td = 0, Rd = 0 ;  at every interface i:  m2 = 1/(1 - Rd*Rupd[i])
//         direct = F0*Tb ; diffuse = F0*((Td + (Tb*Rup[i])*Rd)*m2)
//         up = F0*((Tb*Rup[i] + Td*Rupd[i])*m2) ; down = direct + diffuse
//         through level i:  m3 = 1/(1 - Rd*Rdif_i)
//         Td = Tb*Tdp_i + Tdif_i*((Td + (Tb*Rd)*Rdir_i)*m3) ; Rd = Rdif_i + Tdif_i*((Tdif_i*Rd)*m3)
//         Tb = Tb*D_i
// Against the two-stream equations themselves (tests/two_stream_ode_cases.py solves them without
// these closed forms) the layer is exact to rounding, except: the conservative branch neglects up
// to its criterion (measured 4.8e-11 of F0 per layer); and inside the guard |1 - k*mu0| <
// kTwoStreamResonance the layer is solved at the moved mu0, which puts Rdir and Tdp off by up to
// 0.12*(1e-4 - |1 - k*mu0|) of F0 (measured, g_c <= 0.9): 1.2e-5 of F0 at k*mu0 = 1 under
// mu0 = 1, falling linearly to 0 at the guard's edges.  DESIGN section 12 names the repair.
//
// two_stream_layer is the layer written once; both kernels call it.  They run on path.h's sweep
// skeleton, whole paths only: two_stream_up_kernel sweeps surface -> space with Rup and Rupd in
// registers and writes them to the work rows at the interface above each level;
// two_stream_down_kernel, queued behind it on the same stream, sweeps space -> surface with Tb,
// Td, Rd and F0 in registers, reads beta again and recomputes the layer (three exp, one expm1, one
// sqrt, about eight divisions per element) instead of reading five stored quantities (80 B per
// element beside beta's 8 B), reads the work rows and stores the flux rows asked for; the lane that
// starts a path writes the rows of interface 0.  The level's
// scalars and mu0 are the same for the whole wavefront.
// kSpectral (lbl_path_two_stream_spectral): tau_c, w_c and h_c of a level are no level scalars but
// come per grid point from the scatterer's knot table (scatterer.h): a lane finds where its
// columns lie among the knots once, before its sweep, reads the six knot values of the level's
// three rows per column and level, interpolates and limits them, forms w_c = omega_c*tau_c and
// h_c = w_c*g_c and calls the same two_stream_layer.  Without kSpectral nothing of this is read
// or compiled: the grey kernels are as they were.  Going up the spectral kernel keeps four rows in
// flight (kTwoStreamSpectralUpAhead): with eight it spills scalar registers.
// rayleigh_row_kernel fills sigma(nu) [m2] once per column: Bucholtz (1995) with lambda = 1e4/nu
// in um, sigma = 1e-4*A*lambda^-(B + C*lambda + D/lambda) formed as (1e-4*A)*exp(-(e*log(lambda))),
// 0 for nu <= 0; or the caller's values as they are.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "path.h"
#include "scatterer.h"

namespace lbl {

constexpr double kTwoStreamConservative = 1e-10;    // k2*(1 + t*t) at most: the conservative branch
constexpr double kTwoStreamResonance = 1e-4;        // |1 - k*mu0| below which mu0 is moved off 1/k
constexpr int kTwoStreamLevelWords = 5;             // s_l, c_l, tau_c, w_c, h_c per level
constexpr int kTwoStreamUpAhead = kPathAhead;       // rows of beta in flight per lane, going up
constexpr int kTwoStreamDownAhead = 1;              // going down: more rows spill scalar registers
constexpr int kTwoStreamSpectralUpAhead = 4;        // kSpectral, going up: 8 spill scalar registers

struct PathTwoStream : PathLevels
{
    const double * level;       // [count][5]: s_l, c_l, tau_c, w_c, h_c of flat level first + i
    const double * mu0;         // [paths of the run]: cosine of the solar zenith angle
    const double * albedo;      // [paths of the run]: scalar albedo (without albedo_rows)
    int table_path;             // path of mu0[0] / albedo[0]
    const double * solar;       // [columns]: S on the grid
    const double * sigma;       // [columns]: the Rayleigh cross-section [m2], or null (none)
    const double * albedo_rows; // [paths][stride]: A per path and column, or null
    double * work;              // [count][2][stride]: Rup, Rupd at the interface above each level
    double * level_out[4];      // up, down, direct, diffuse at the interface below each level
    double * top_out[4];        // [paths][stride]: the same at interface 0 (null: not wanted)
};

// lbl_path_two_stream_spectral's: the same with the scatterer's knot table, which replaces tau_c,
// w_c and h_c of the level rows (0 there) per grid point.
struct PathTwoStreamSpectral : PathTwoStream
{
    ScattererKnots scatterer;
};

template <bool kSpectral>
using TwoStreamArguments = std::conditional_t<kSpectral, PathTwoStreamSpectral, PathTwoStream>;

// What a layer does to light: its diffuse reflectance and transmittance, the reflectance for the
// direct beam, the diffuse part of the transmitted beam and the beam's own transmittance.
struct TwoStreamLayer
{
    double rdif, tdif, rdir, tdp, d;
};

// The layer of one level and grid point (the formulas in the head of this file).  s .. h_c: the
// level's table row; b: beta; sigma: the Rayleigh cross-section.
__device__ __forceinline__ TwoStreamLayer two_stream_layer(double s, double c, double tau_c,
                                                           double w_c, double h_c, double mu0,
                                                           double b, double sigma)
{
    TwoStreamLayer y;
    const double tau_a = s*b;
    const double tau_r = c*sigma;
    const double tau = (tau_a + tau_r) + tau_c;
    if (tau == 0.)
    {
        y.rdif = y.rdir = y.tdp = 0.;
        y.tdif = y.d = 1.;
        return y;
    }
    const double tau_s = tau_r + w_c;
    const double omega = tau_s/tau;
    const double g = tau_s == 0. ? 0. : h_c/tau_s;
    const double f = g*g;
    const double sc = 1. - omega*f;
    const double t = sc*tau;
    const double w = ((1. - f)*omega)/sc;
    const double gp = g/(1. + g);
    const double g2 = (3.*(w*(1. - gp)))/4.;
    const double dif = 2.*(1. - w);
    const double g1 = g2 + dif;
    const double su = g1 + g2;
    const double g3 = (2. - 3.*(mu0*gp))/4.;
    const double g4 = 1. - g3;
    const double k2 = dif*su;
    y.d = exp(-t/mu0);
    if (k2*(1. + t*t) <= kTwoStreamConservative)
    {
        const double x = g1*t;
        y.rdif = x/(1. + x);
        y.tdif = 1./(1. + x);
        y.rdir = (x + (g3 - g1*mu0)*(-expm1(-t/mu0)))/(1. + x);
        y.tdp = (1. - y.rdir) - y.d;
        return y;
    }
    const double k = sqrt(k2);
    double m = mu0;
    double x = k*m;
    double dm = y.d;
    if (fabs(1. - x) < kTwoStreamResonance)
    {
        m = (x >= 1. ? (1. + kTwoStreamResonance) : (1. - kTwoStreamResonance))/k;
        x = k*m;
        dm = exp(-t/m);
    }
    const double e = exp(-(k*t));
    const double e2 = e*e;
    const double o1 = -expm1(-(2.*(k*t)));
    const double den = k*(1. + e2) + g1*o1;
    const double q = ((1. - x)*(1. + x))*den;
    y.rdif = (g2*o1)/den;
    y.tdif = (2.*(k*e))/den;
    const double a1 = g1*g4 + g2*g3;
    const double a2 = g1*g3 + g2*g4;
    y.rdir = w*((1. - x)*(a2 + k*g3) - ((1. + x)*(a2 - k*g3))*e2 -
                (2.*(k*(g3 - a2*m)))*(e*dm))/q;
    const double ttot = dm*(1. - w*((1. + x)*(a1 + k*g4) - ((1. - x)*(a1 - k*g4))*e2)/q) +
        w*((2.*(k*(g4 + a1*m)))*e)/q;
    y.tdp = ttot - dm;
    return y;
}

// The lane's columns of sigma (zeros without a row) and of the albedo of path p.
template <bool kVector>
__device__ __forceinline__ void two_stream_columns(const PathTwoStream & a, const PathLane & l,
                                                   double (&sigma)[kPathWidth],
                                                   double (&albedo)[kPathWidth])
{
    if (a.sigma != nullptr)
    {
        path_load<kVector>(a.sigma + l.j, l.width, sigma);
    }
    else
    {
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) sigma[i] = 0.;
    }
    if (a.albedo_rows != nullptr)
    {
        path_load<kVector>(a.albedo_rows + (long long)l.p*a.stride + l.j, l.width, albedo);
    }
    else
    {
        const double scalar = a.albedo[l.p - a.table_path];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) albedo[i] = scalar;
    }
}

// F0*v at offset `at` of `out` (null: nothing).
template <bool kVector>
__device__ __forceinline__ void two_stream_store(double * out, long long at, int width,
                                                 const double (&v)[kPathWidth])
{
    if (out != nullptr) path_store<kVector>(out + at, width, v);
}

// The four fluxes of an interface where the light from above is (tb, td, rd) and what lies below
// reflects (rup, rupd), stored at offset `at` of the rows `out` (null: not wanted).
template <bool kVector>
__device__ __forceinline__ void two_stream_interface(
    double * const (&out)[4], long long at, int width, const double (&f0)[kPathWidth],
    const double (&tb)[kPathWidth], const double (&td)[kPathWidth],
    const double (&rd)[kPathWidth], const double (&rup)[kPathWidth],
    const double (&rupd)[kPathWidth])
{
    double up[kPathWidth], down[kPathWidth], direct[kPathWidth], diffuse[kPathWidth];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        const double m2 = 1./(1. - rd[i]*rupd[i]);
        direct[i] = f0[i]*tb[i];
        diffuse[i] = f0[i]*((td[i] + (tb[i]*rup[i])*rd[i])*m2);
        up[i] = f0[i]*((tb[i]*rup[i] + td[i]*rupd[i])*m2);
        down[i] = direct[i] + diffuse[i];
    }
    two_stream_store<kVector>(out[0], at, width, up);
    two_stream_store<kVector>(out[1], at, width, down);
    two_stream_store<kVector>(out[2], at, width, direct);
    two_stream_store<kVector>(out[3], at, width, diffuse);
}

// kSpectral: where the lane's columns lie among the scatterer's knots.
template <bool kVector>
__device__ __forceinline__ ScattererLane two_stream_knots(const PathTwoStreamSpectral & a,
                                                          const PathLane & l)
{
    double nu[kPathWidth];
    path_load<kVector>(a.scatterer.nu + l.j, l.width, nu);
    return scatterer_lane(a.scatterer, nu);
}

// kSpectral: the layer of one level and grid point with the scatterer interpolated from the
// level's three knot rows `optics`: tau_c, omega_c and g_c at the column, then w_c = omega_c*tau_c
// and h_c = w_c*g_c as the host forms them for the grey scatterer.
__device__ __forceinline__ TwoStreamLayer two_stream_spectral_layer(
    double s, double c, const double * optics, int n_knots, int j, double u, double mu0, double b,
    double sigma)
{
    const double tau_c = scatterer_value(optics, j, u);
    const double omega_c = scatterer_value(optics + n_knots, j, u);
    const double g_c = scatterer_value(optics + 2*n_knots, j, u);
    const double w_c = omega_c*tau_c;
    return two_stream_layer(s, c, tau_c, w_c, w_c*g_c, mu0, b, sigma);
}

// grid and kVector as for path_sweep_kernel; a.from_last is the order of this sweep, surface to
// space.  Whole paths: every lane starts and finishes its path.  kSpectral: the scatterer comes
// from its knot table (scatterer.h) in place of the level rows; without it nothing of that is read.
template <bool kVector, bool kSpectral = false>
__global__ __launch_bounds__(kPathThreads) void two_stream_up_kernel(
    TwoStreamArguments<kSpectral> a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const double * level = a.level + (long long)l.index0*kTwoStreamLevelWords;
    const int width = l.width;
    const double mu0 = a.mu0[l.p - a.table_path];

    double sigma[kPathWidth], rup[kPathWidth], rupd[kPathWidth];
    two_stream_columns<kVector>(a, l, sigma, rup);
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i) rupd[i] = rup[i];
    ScattererLane knots;
    if constexpr (kSpectral) knots = two_stream_knots<kVector>(a, l);

    const auto step = [&](int k, const double (&b)[kPathWidth], long long at) {
        const double * row = level + (long long)(k*l.direction)*kTwoStreamLevelWords;
        const double s = row[0], c = row[1], tau_c = row[2], w_c = row[3], h_c = row[4];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            TwoStreamLayer y;
            if constexpr (kSpectral)
            {
                y = two_stream_spectral_layer(
                    s, c, scatterer_rows(a.scatterer, l.index0 + k*l.direction),
                    a.scatterer.n_knots, knots.j[i], knots.u[i], mu0, b[i], sigma[i]);
            }
            else
            {
                y = two_stream_layer(s, c, tau_c, w_c, h_c, mu0, b[i], sigma[i]);
            }
            const double m1 = 1./(1. - y.rdif*rupd[i]);
            const double up = y.rdir + y.tdif*((y.tdp*rupd[i] + y.d*rup[i])*m1);
            rupd[i] = y.rdif + y.tdif*((y.tdif*rupd[i])*m1);
            rup[i] = up;
        }
        double * work = a.work + (2*at - l.j);
        path_store<kVector>(work, width, rup);
        path_store<kVector>(work + a.stride, width, rupd);
    };
    if constexpr (kSpectral)
    {
        path_levels<kTwoStreamSpectralUpAhead, kVector>(a, l, step);
    }
    else
    {
        path_levels<kTwoStreamUpAhead, kVector>(a, l, step);
    }
}

// grid and kVector as for path_sweep_kernel; a.from_last is the Sun's order, space to surface.
// kSpectral as for two_stream_up_kernel.
template <bool kVector, bool kSpectral = false>
__global__ __launch_bounds__(kPathThreads) void two_stream_down_kernel(
    TwoStreamArguments<kSpectral> a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const double * level = a.level + (long long)l.index0*kTwoStreamLevelWords;
    const int width = l.width;
    const double mu0 = a.mu0[l.p - a.table_path];

    double sigma[kPathWidth], albedo[kPathWidth], f0[kPathWidth];
    two_stream_columns<kVector>(a, l, sigma, albedo);
    path_load<kVector>(a.solar + l.j, width, f0);
    double tb[kPathWidth], td[kPathWidth], rd[kPathWidth], rup[kPathWidth], rupd[kPathWidth];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        f0[i] = mu0*f0[i];
        tb[i] = 1.;
        td[i] = rd[i] = 0.;
    }
    // Interface 0: what the whole path reflects is in the work rows of the first level.
    {
        const double * work = a.work + (2*l.level0 - l.j);
        path_load<kVector>(work, width, rup);
        path_load<kVector>(work + a.stride, width, rupd);
        two_stream_interface<kVector>(a.top_out, (long long)l.p*a.stride + l.j, width, f0, tb,
                                      td, rd, rup, rupd);
    }
    ScattererLane knots;
    if constexpr (kSpectral) knots = two_stream_knots<kVector>(a, l);
    path_levels<kTwoStreamDownAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth],
                                                          long long at) {
        const double * row = level + (long long)(k*l.direction)*kTwoStreamLevelWords;
        const double s = row[0], c = row[1], tau_c = row[2], w_c = row[3], h_c = row[4];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            TwoStreamLayer y;
            if constexpr (kSpectral)
            {
                y = two_stream_spectral_layer(
                    s, c, scatterer_rows(a.scatterer, l.index0 + k*l.direction),
                    a.scatterer.n_knots, knots.j[i], knots.u[i], mu0, b[i], sigma[i]);
            }
            else
            {
                y = two_stream_layer(s, c, tau_c, w_c, h_c, mu0, b[i], sigma[i]);
            }
            const double m3 = 1./(1. - rd[i]*y.rdif);
            td[i] = tb[i]*y.tdp + y.tdif*((td[i] + (tb[i]*rd[i])*y.rdir)*m3);
            rd[i] = y.rdif + y.tdif*((y.tdif*rd[i])*m3);
            tb[i] = tb[i]*y.d;
        }
        // What lies below this level: the next level's work rows, or the surface.
        if (k + 1 < l.n)
        {
            const double * work = a.work + (2*(at + l.row_step) - l.j);
            path_load<kVector>(work, width, rup);
            path_load<kVector>(work + a.stride, width, rupd);
        }
        else
        {
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i) rup[i] = rupd[i] = albedo[i];
        }
        two_stream_interface<kVector>(a.level_out, at, width, f0, tb, td, rd, rup, rupd);
    });
}

// Bucholtz (1995), table 3: sigma = A*lambda^-(B + C*lambda + D/lambda) [cm2], lambda [um].
constexpr double kRayleighSplit = 0.5;      // lambda <= 0.5 um: the first row
constexpr double kRayleighShort[4] = {3.01577e-28, 3.55212, 1.35579, 0.11563};
constexpr double kRayleighLong[4] = {4.01061e-28, 3.99668, 1.10298e-3, 2.71393e-2};

struct RayleighRow
{
    const double * nu;          // [columns]: the grid [cm-1]
    long long columns;
    const double * value;       // [columns]: the caller's cross-sections [m2], or null (the fit)
    double * row;               // [columns]
};

__device__ __forceinline__ double rayleigh_cross_section(double nu)
{
    if (!(nu > 0.)) return 0.;
    const double lambda = 1e4/nu;
    const bool is_short = lambda <= kRayleighSplit;
    const double a = is_short ? kRayleighShort[0] : kRayleighLong[0];
    const double b = is_short ? kRayleighShort[1] : kRayleighLong[1];
    const double c = is_short ? kRayleighShort[2] : kRayleighLong[2];
    const double d = is_short ? kRayleighShort[3] : kRayleighLong[3];
    const double e = (b + c*lambda) + d/lambda;
    return (1e-4*a)*exp(-(e*log(lambda)));
}

// grid (columns / (kPathThreads*kPathWidth)).  kVector: the grid, the values and the row are
// 16-byte aligned.
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void rayleigh_row_kernel(RayleighRow a)
{
    const long long j = ((long long)blockIdx.x*kPathThreads + threadIdx.x)*kPathWidth;
    if (j >= a.columns) return;
    const int width = (int)(a.columns - j < kPathWidth ? a.columns - j : kPathWidth);
    double out[kPathWidth];
    if (a.value != nullptr)
    {
        path_load<kVector>(a.value + j, width, out);
    }
    else
    {
        double nu[kPathWidth];
        path_load<kVector>(a.nu + j, width, nu);
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) out[i] = rayleigh_cross_section(nu[i]);
    }
    path_store<kVector>(a.row + j, width, out);
}

}  // namespace lbl
