// Sunlight scattered to a sensor (Spectroscopy.compute_solar_radiance, lbl_path_solar_radiance):
// the radiance a viewer above the atmosphere sees along one zenith cosine and one azimuth per
// path, from the two-stream source-function technique (Toon et al. 1989): the fluxes of
// lbl_path_two_stream (twostream.h) are the source of multiply scattered light, the singly
// scattered direct beam is treated with the true phase functions (the TMS correction of Nakajima
// & Tanaka 1988), and the transfer equation is integrated exactly along the viewing direction
// through every level, over the "total" absorption block in HBM.  The TU builds with
// -ffp-contract=off: every product, sum and quotient below is rounded as written.
//
// Inputs.  beta, the paths, the level row (s_l, c_l, tau_c, w_c, h_c), sigma(nu), A, F0 = mu0*S
// and every layer scalar are twostream.h's, bit for bit:
//   tau_a = s_l*beta ; tau_R = c_l*sigma ; tau = (tau_a + tau_R) + tau_c ; tau_s = tau_R + w_c
//   omega = tau_s/tau ; g = h_c/tau_s ; f = g*g ; sc = 1 - omega*f ; t = sc*tau
//   w = ((1 - f)*omega)/sc ; gp = g/(1 + g) ; g2 = (3*(w*(1 - gp)))/4 ; dif = 2*(1 - w)
//   g1 = g2 + dif ; su = g1 + g2 ; g3 = (2 - 3*(mu0*gp))/4 ; g4 = 1 - g3 ; k2 = dif*su
//   a1 = g1*g4 + g2*g3 ; a2 = g1*g3 + g2*g4
//   conservative, where k2*(1 + t*t) <= kTwoStreamConservative: m = mu0
//   general: k = sqrt(k2) ; m = mu0 ; x = k*m
//     if |1 - x| < kTwoStreamResonance: m = (x >= 1 ? (1 + 1e-4) : (1 - 1e-4))/k ; x = k*m
//     E = exp(-(k*t))
//   Dm = exp(-t/m)
// Inside the guard around k*mu0 = 1 the level uses the moved cosine m for the beam, in its
// particular solution and in its single scattering, as the flux rows do.
// mu in (0, 1]: the viewing zenith cosine, and cosT in [-1, 1]: the cosine of the scattering
// angle, one each per path.  up[i], diffuse[i], direct[i]: lbl_path_two_stream's fluxes at
// interface i; level i lies between interfaces i (space side) and i + 1, interface 0 faces space,
// and direct[0] = F0 and diffuse[0] = 0 are constants, not read.
// Model.  tau' in [0, t] is measured from the level's space-side face and S_i = direct[i]:
//   Dv = exp(-t/mu) ; a = (3*(gp*mu))/2
//   beam       B(tau') = S_i*exp(-tau'/m)
//   diffuse    F+(tau'), F-(tau'): the two-stream solution in the level (below)
//   source     J(tau') = (w/(2 pi))*[F+(tau')(1 + a) + F-(tau')(1 - a)]
//                      + ((omega/sc)*Pmix/(4 pi))*(S_i/m)*exp(-tau'/m)
//   Pmix = (tau_R*PR + w_c*PH)/tau_s ;  PR = (3/4)(1 + cosT^2)
//   PH = (1 - gc^2)/(1 + gc^2 - 2 gc cosT)^(3/2),  gc = h_c/w_c  (0 where w_c == 0)
//   transfer   I_top = I_bot*Dv + Integral_0^t J(tau') exp(-tau'/mu) dtau'/mu
// The first term of J is the two-stream phase function 1 + 3 g' mu mu' with hemispherically
// isotropic I+- = F+-/pi; the second is the direct beam B/m scattered once by the unscaled
// optics (omega dtau = (omega/sc) dtau').  F+- solve the Meador-Weaver equations
//   dF+/dtau' = g1 F+ - g2 F- - w g3 (B/m) ;  dF-/dtau' = g2 F+ - g1 F- + w g4 (B/m)
// whose particular solution Z+- exp(-tau'/m) has, with X = (1 - x)*(1 + x) (X = 1, conservative):
//   ws = w*S_i ; Z+ = (ws*(g3 - a2*m))/X ; Z- = -((ws*(g4 + a1*m))/X)
//   u1 = up[i+1] - Z+*Dm ; d0 = diffuse[i] - Z-
//   bm = (m/(m + mu))*(-expm1(-(t/m + t/mu)))   (no difference of exponentials: thin levels)
//   I_top = I_bot*Dv + (w/(2 pi))*C + (((omega/sc)*Pmix)/(4 pi))*((S_i/m)*bm)
// general:
//   Gamma = g2/(g1 + k) ; n = 1 - (Gamma*E)*(Gamma*E)
//   P = (u1 - (Gamma*E)*d0)/n ; Q = (d0 - (Gamma*E)*u1)/n
//     (F+ = P e^{-k(t - tau')} + Gamma Q e^{-k tau'} + Z+ e^{-tau'/m}
//      F- = Gamma P e^{-k(t - tau')} + Q e^{-k tau'} + Z- e^{-tau'/m})
//   C = P*((1 + a) + Gamma*(1 - a))*h + Q*(Gamma*(1 + a) + (1 - a))*((1 - E*Dv)/(1 + k*mu))
//       + (Z+*(1 + a) + Z-*(1 - a))*bm
//   h = (E - Dv)/(1 - k mu), formed without its pole and without overflow (thermal_radiance.h):
//     y = ((1 - k*mu)*t)/mu ; phi(z) = -expm1(-z)/z for z > 0, phi(0) = 1
//     h = E*((t/mu)*phi(y)) for y >= 0 ; h = Dv*((t/mu)*phi(-y)) for y < 0
// conservative:
//   x = g1*t ; N = (u1 - d0)/(1 + x) ; Ev = -expm1(-t/mu)
//     (F+ = u1 - g1 N (t - tau') + Z+ e^{-tau'/m} ; F- = d0 + g1 N tau' + Z- e^{-tau'/m})
//   C = ((u1 + d0) - x*N + a*N)*Ev + (2*(g1*N))*(mu*W) + (Z+*(1 + a) + Z-*(1 - a))*bm
//   W = Ev - (t/mu)*Dv, formed without its cancellation as
//     W = (t/mu)*(Ev - linear_weight(t/mu, Ev))        (radiance.h's w = 1 - Ev/(t/mu))
// Special levels.  tau == 0: the identity.  tau_s == 0: I_top = I_bot*exp(-tau/mu).  A call
// without a Rayleigh row in a level with w_c == 0 has tau_s == 0 in every column: that is decided
// once for the whole wavefront, and the level loads no flux row.
// Surface and result.  I_L = A*((direct[L] + diffuse[L])/pi): a Lambertian surface.  The result is
// I at interface 0.
//
// solar_view_kernel runs on path.h's sweep skeleton, whole paths only, surface -> space with I in
// registers.  mu, mu0, cosT, PR, PH and the level's row are the same for the whole wavefront.  A
// lane reads sigma, S and the albedo once; per level beta; in a scattering level also up_rows of
// the level and direct_rows and diffuse_rows of the next level towards space (F0 and 0 at the
// path's last step), and it restates the layer scalars: two_stream_layer is not touched.  It
// writes one row per path.
//
// kSpectral (lbl_path_solar_radiance_spectral; include/lbl_amd_scatterer_radiance.h): tau_c, w_c
// and h_c of a level come per grid point from the scatterer's knot table (scatterer.h) in place of
// the level row, as in twostream.h's spectral kernels and through the same scatterer_lane, so that
// the view and the flux sweeps before it place every column among the knots identically.  Per
// level and column the six knot values are loaded together ahead of the level's arithmetic; then
// w_c = omega_c*tau_c, h_c = w_c*g_c, PH from gc = h_c/w_c -- from the products, as the grey kernel
// forms it, so that a flat table gives its bits -- and the same solar_view_level.  gc: with g_c <=
// 1 - 2^-53 and w_c a normal number, w_c*g_c lies at least half an ulp of w_c below w_c and rounds
// below it, and the quotient of two doubles h_c < w_c rounds to at most 1 - 2^-53; a subnormal w_c
// can give h_c == w_c, so gc is limited to 1 - 2^-53 (kSolarViewMaxAsymmetry), which changes no
// value below it.  The wave-uniform short cut is taken where the call has no Rayleigh row and no
// knot of the level scatters (the `scatters` word lbl_path_thermal_two_stream_spectral uses too).
// Without kSpectral nothing of this is read or compiled.
#pragma once

#include <hip/hip_runtime.h>

#include "path.h"
#include "radiance.h"
#include "thermal_radiance.h"
#include "twostream.h"

namespace lbl {

constexpr int kSolarViewAhead = 1;      // rows of beta in flight per lane

// lbl_path_solar_radiance's: PathTwoStream's table, Sun and surface (work, level_out and top_out
// are not used), with the view, the flux rows and the output.
struct PathSolarView : PathTwoStream
{
    const double * mu;          // [paths of the run]: the viewing zenith cosine
    const double * cos_theta;   // [paths of the run]: the cosine of the scattering angle
    const double * up;          // [count][stride]: up at the interface below each level
    const double * direct;      // [count][stride]: direct there
    const double * diffuse;     // [count][stride]: diffuse there
    double * rad;               // [paths][stride]: I at interface 0
};

// lbl_path_solar_radiance_spectral's: PathTwoStreamSpectral's table and knots with the same view,
// flux rows and output.
struct PathSolarViewSpectral : PathTwoStreamSpectral
{
    const double * mu;
    const double * cos_theta;
    const double * up;
    const double * direct;
    const double * diffuse;
    double * rad;
    const double * scatters;    // [count]: 0 where every knot of flat level first + i has
                                // omega_c*tau_c == 0, else 1
};

template <bool kSpectral>
using SolarViewArguments = std::conditional_t<kSpectral, PathSolarViewSpectral, PathSolarView>;

constexpr double kSolarViewMaxAsymmetry = 1. - 0x1p-53;     // the largest double below 1

// PH of a level's scatterer at cosT (0 where the level holds none).
__device__ __forceinline__ double solar_view_henyey(double w_c, double h_c, double cos_theta)
{
    if (w_c == 0.) return 0.;
    const double gc = h_c/w_c;
    const double den = (1. + gc*gc) - (2.*gc)*cos_theta;
    return (1. - gc*gc)/(den*sqrt(den));
}

// kSpectral: the same of an element's interpolated scatterer, with gc kept below 1 (the head of
// this file).
__device__ __forceinline__ double solar_view_henyey_limited(double w_c, double h_c,
                                                            double cos_theta)
{
    if (w_c == 0.) return 0.;
    const double gc = fmin(h_c/w_c, kSolarViewMaxAsymmetry);
    const double den = (1. + gc*gc) - (2.*gc)*cos_theta;
    return (1. - gc*gc)/(den*sqrt(den));
}

// I at the space-side face of a level from `rad` at its surface-side face (the formulas in the
// head of this file).  s .. h_c: the level's table row; mu0, mu: the Sun's and the view's cosine;
// pr, ph: the two phase functions at the scattering angle; b: beta; sigma: the Rayleigh
// cross-section; up1: up at the level's surface-side interface; direct0, diffuse0: the fluxes at
// its space-side interface.
__device__ __forceinline__ double solar_view_level(double s, double c, double tau_c, double w_c,
                                                   double h_c, double mu0, double mu, double pr,
                                                   double ph, double b, double sigma, double up1,
                                                   double direct0, double diffuse0, double rad)
{
    const double tau_a = s*b;
    const double tau_r = c*sigma;
    const double tau = (tau_a + tau_r) + tau_c;
    if (tau == 0.) return rad;
    const double tau_s = tau_r + w_c;
    if (tau_s == 0.) return rad*exp(-tau/mu);
    const double omega = tau_s/tau;
    const double g = h_c/tau_s;
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
    const double a1 = g1*g4 + g2*g3;
    const double a2 = g1*g3 + g2*g4;
    const double z = t/mu;
    const double dv = exp(-z);
    const double a = (3.*(gp*mu))/2.;
    const double pmix = (tau_r*pr + w_c*ph)/tau_s;
    const double ws = w*direct0;
    double m = mu0;
    double cc, bm;
    if (k2*(1. + t*t) <= kTwoStreamConservative)
    {
        const double zp = ws*(g3 - a2*m);
        const double zm = -(ws*(g4 + a1*m));
        const double dm = exp(-t/m);
        const double u1 = up1 - zp*dm;
        const double d0 = diffuse0 - zm;
        bm = (m/(m + mu))*(-expm1(-(t/m + z)));
        const double ev = -expm1(-z);
        const double x = g1*t;
        const double n = (u1 - d0)/(1. + x);
        const double big_w = z*(ev - linear_weight(z, ev));
        cc = ((u1 + d0) - x*n + a*n)*ev + (2.*(g1*n))*(mu*big_w) +
             (zp*(1. + a) + zm*(1. - a))*bm;
    }
    else
    {
        const double k = sqrt(k2);
        double x = k*m;
        if (fabs(1. - x) < kTwoStreamResonance)
        {
            m = (x >= 1. ? (1. + kTwoStreamResonance) : (1. - kTwoStreamResonance))/k;
            x = k*m;
        }
        const double dm = exp(-t/m);
        const double e = exp(-(k*t));
        const double big_x = (1. - x)*(1. + x);
        const double zp = (ws*(g3 - a2*m))/big_x;
        const double zm = -((ws*(g4 + a1*m))/big_x);
        const double u1 = up1 - zp*dm;
        const double d0 = diffuse0 - zm;
        bm = (m/(m + mu))*(-expm1(-(t/m + z)));
        const double gamma = g2/(g1 + k);
        const double ge = gamma*e;
        const double n = 1. - ge*ge;
        const double p = (u1 - ge*d0)/n;
        const double q = (d0 - ge*u1)/n;
        const double y = ((1. - k*mu)*t)/mu;
        const double h = y >= 0. ? e*(z*thermal_view_phi(y)) : dv*(z*thermal_view_phi(-y));
        cc = p*((1. + a) + gamma*(1. - a))*h +
             q*(gamma*(1. + a) + (1. - a))*((1. - e*dv)/(1. + k*mu)) +
             (zp*(1. + a) + zm*(1. - a))*bm;
    }
    return rad*dv + (w/(2.*kFluxPi))*cc + (((omega/sc)*pmix)/(4.*kFluxPi))*((direct0/m)*bm);
}

// grid and kVector as for path_sweep_kernel; a.from_last is the order of this sweep, surface to
// space.  Whole paths: every lane starts and finishes its path.  kSpectral: the scatterer comes
// from its knot table (scatterer.h) in place of the level rows; without it nothing of that is read.
template <bool kVector, bool kSpectral = false>
__global__ __launch_bounds__(kPathThreads) void solar_view_kernel(SolarViewArguments<kSpectral> a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const int width = l.width;
    const double * level = a.level + (long long)l.index0*kTwoStreamLevelWords;
    const double mu0 = a.mu0[l.p - a.table_path];
    const double mu = a.mu[l.p - a.table_path];
    const double cos_theta = a.cos_theta[l.p - a.table_path];
    const double pr = (3.*(1. + cos_theta*cos_theta))/4.;

    double sigma[kPathWidth], f0[kPathWidth], rad[kPathWidth];
    // The surface: what it reflects of the light that reaches it -- the direct and diffuse rows
    // of the first level of the sweep.
    {
        double albedo[kPathWidth], direct[kPathWidth], diffuse[kPathWidth];
        two_stream_columns<kVector>(a, l, sigma, albedo);
        path_load<kVector>(a.solar + l.j, width, f0);
        path_load<kVector>(a.direct + l.level0, width, direct);
        path_load<kVector>(a.diffuse + l.level0, width, diffuse);
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            f0[i] = mu0*f0[i];
            rad[i] = albedo[i]*((direct[i] + diffuse[i])/kFluxPi);
        }
    }

    ScattererLane knots;
    if constexpr (kSpectral) knots = two_stream_knots<kVector>(a, l);

    path_levels<kSolarViewAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth],
                                                      long long at) {
        const double * row = level + (long long)(k*l.direction)*kTwoStreamLevelWords;
        if constexpr (kSpectral)
        {
            const double s = row[0], c = row[1];
            const int index = l.index0 + k*l.direction;
            const int m = a.scatterer.n_knots;
            const double * rows = scatterer_rows(a.scatterer, index);
            if (a.sigma == nullptr && a.scatters[index] == 0.)
            {
#pragma unroll
                for (int i = 0; i < kPathWidth; ++i)
                {
                    const double tau_c = scatterer_value(rows, knots.j[i], knots.u[i]);
                    const double tau_a = s*b[i];
                    const double tau = tau_a + tau_c;
                    rad[i] = rad[i]*exp(-tau/mu);
                }
                return;
            }
            double tau_c[kPathWidth], omega_c[kPathWidth], g_c[kPathWidth];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                tau_c[i] = scatterer_value(rows, knots.j[i], knots.u[i]);
                omega_c[i] = scatterer_value(rows + m, knots.j[i], knots.u[i]);
                g_c[i] = scatterer_value(rows + 2*m, knots.j[i], knots.u[i]);
            }
            // The grey branch's loads, restated: moved into a function that both branches
            // call, they change the instructions of the grey instantiations.
            double up1[kPathWidth], direct0[kPathWidth], diffuse0[kPathWidth];
            path_load<kVector>(a.up + at, width, up1);
            if (k + 1 < l.n)
            {
                path_load<kVector>(a.direct + (at + l.row_step), width, direct0);
                path_load<kVector>(a.diffuse + (at + l.row_step), width, diffuse0);
            }
            else
            {
#pragma unroll
                for (int i = 0; i < kPathWidth; ++i)
                {
                    direct0[i] = f0[i];
                    diffuse0[i] = 0.;
                }
            }
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double w_c = omega_c[i]*tau_c[i];
                const double h_c = w_c*g_c[i];
                const double ph = solar_view_henyey_limited(w_c, h_c, cos_theta);
                rad[i] = solar_view_level(s, c, tau_c[i], w_c, h_c, mu0, mu, pr, ph, b[i],
                                          sigma[i], up1[i], direct0[i], diffuse0[i], rad[i]);
            }
            return;
        }
        const double s = row[0], c = row[1], tau_c = row[2], w_c = row[3], h_c = row[4];
        if (a.sigma == nullptr && w_c == 0.)
        {
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double tau_a = s*b[i];
                const double tau = tau_a + tau_c;
                rad[i] = rad[i]*exp(-tau/mu);
            }
            return;
        }
        // Below this level: its own rows; above it: the next level's, or space.
        double up1[kPathWidth], direct0[kPathWidth], diffuse0[kPathWidth];
        path_load<kVector>(a.up + at, width, up1);
        if (k + 1 < l.n)
        {
            path_load<kVector>(a.direct + (at + l.row_step), width, direct0);
            path_load<kVector>(a.diffuse + (at + l.row_step), width, diffuse0);
        }
        else
        {
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                direct0[i] = f0[i];
                diffuse0[i] = 0.;
            }
        }
        const double ph = solar_view_henyey(w_c, h_c, cos_theta);
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            rad[i] = solar_view_level(s, c, tau_c, w_c, h_c, mu0, mu, pr, ph, b[i], sigma[i],
                                      up1[i], direct0[i], diffuse0[i], rad[i]);
        }
    });

    path_store<kVector>(a.rad + ((long long)l.p*a.stride + l.j), width, rad);
}

}  // namespace lbl
