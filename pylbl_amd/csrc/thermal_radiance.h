// Sounder radiances through clouds (Spectroscopy.compute_thermal_radiance,
// lbl_path_thermal_radiance): the radiance a viewer above the atmosphere sees along one zenith
// cosine per path, from the two-stream source-function technique (Toon et al. 1989): the fluxes of
// lbl_path_thermal_two_stream (twostream_thermal.h) are the scattering source, and the transfer
// equation is integrated exactly along the viewing direction through every level, over the
// "total" absorption block in HBM.  The TU builds with -ffp-contract=off: every product, sum and
// quotient below is rounded as written.
//
// Inputs.  Per level l the table row is (s_l, tau_c, w_c, g_c, T_l) and D the diffusivity factor:
// twostream_thermal.h's, bit for bit, with its tau, the clear/cloudy wave-uniform branch and
//   omega = w_c/tau ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc
//   g2 = (D*(w*(1 - gp)))/2 ; dif = D*(1 - w) ; g1 = g2 + dif ; su = g1 + g2 ; k2 = dif*su
//   conservative, where k2*(1 + t*t) <= 1e-10 ; general: k = sqrt(k2) ; E = exp(-(k*t))
// mu in (0, 1]: the viewing zenith cosine, one per path.  up[i], down[i]: the two-stream fluxes at
// interface i; level i lies between interfaces i and i + 1, interface 0 faces space and down[0] = 0
// is a constant, not read.  B = planck(nu, c1nu3, c2nu, T_l) and piB = kFluxPi*B.
//   gp = g_c/(1 + g_c) ; a = (3*(gp*mu))/2
// Model.  Within a level the source is J(tau) = B + (w/(2 pi))*[f+(tau)(1 + a) + f-(tau)(1 - a)]
// with f+- = F+- - piB: the two-stream phase function 1 + 3 g' mu mu' with hemispherically
// isotropic I+- = F+-/pi; the (1 - w)B term and the scattered piB terms sum to B.  With
//   u1 = up[i+1] - piB ; d0 = down[i] - piB ; Dm = exp(-t/mu) ; Em = -expm1(-t/mu)
// the level maps the radiance entering its surface-side face, I_bot, to
//   I_top = I_bot*Dm + B*Em + (w/(2 pi))*C
// clear level (w_c == 0, the same for the whole wavefront):  x = tau/mu and C = 0:
//   I_top = I_bot*exp(-x) + B*(-expm1(-x))
//   (path_radiance_kernel's lines: mu = 1 without tau_c gives its bits)
// cloudy, general:
//   Gamma = g2/(g1 + k) ; n = 1 - (Gamma*E)*(Gamma*E)
//   P = (u1 - (Gamma*E)*d0)/n ; Q = (d0 - (Gamma*E)*u1)/n
//     (f+ = P e^{-k(t - tau)} + Gamma Q e^{-k tau} ; f- = Gamma P e^{-k(t - tau)} + Q e^{-k tau})
//   C = P*((1 + a) + Gamma*(1 - a))*h + Q*(Gamma*(1 + a) + (1 - a))*((1 - E*Dm)/(1 + k*mu))
//   h = (E - Dm)/(1 - k mu), formed without its pole and without overflow:
//     y = ((1 - k*mu)*t)/mu ; phi(z) = -expm1(-z)/z for z > 0, phi(0) = 1
//     h = E*((t/mu)*phi(y)) for y >= 0 ; h = Dm*((t/mu)*phi(-y)) for y < 0
//     (the first form alone is 0*inf where k t is large under a small t/mu)
// cloudy, conservative:
//   x = g1*t ; N = (u1 - d0)/(1 + x)
//     (f+ = u1 - g1 N (t - tau) ; f- = d0 + g1 N tau)
//   C = ((u1 + d0) - x*N + a*N)*Em + (2*(g1*N))*(mu*W)
//   W = Em - (t/mu)*Dm, formed without its cancellation as
//     W = (t/mu)*(Em - linear_weight(t/mu, Em))        (radiance.h's w = 1 - Em/(t/mu))
// Surface and result.  I_L = eps*B(T_s) + (1 - eps)*(down[L]/pi): a Lambertian surface with eps as
// in twostream_thermal.h (a scalar per path, or rows).  The result is I at interface 0; its
// brightness temperature is radiance.h's.
//
// thermal_view_kernel runs on path.h's sweep skeleton, whole paths only, surface -> space with I in
// registers.  mu, a and the level's row are the same for the whole wavefront.  Per level a lane
// reads beta; in a cloudy level also up_rows of the level and down_rows of the next level towards
// space (0 at the path's last step), and it recomputes the layer scalars.  A clear level costs one
// exp, one expm1 and the Planck function and reads no flux rows.  It writes one row per path, and
// the brightness temperature beside it where asked.
//
// kSpectral (lbl_path_thermal_radiance_spectral; include/lbl_amd_scatterer_radiance.h): tau_c,
// w_c and g_c of a level come per grid point from the scatterer's knot table (scatterer.h) in place
// of the level row, as in twostream_thermal.h's spectral kernels and through the same
// scatterer_lane, so that the view and the flux sweeps before it place every column among the
// knots identically.  A level none of whose knots scatters (the `scatters` word of the flux entry)
// is clear for the whole wavefront, with tau = s*beta + tau_c(nu), and reads no flux row.  In a
// level that scatters every element takes thermal_view_cloudy with its own tau_c, w_c =
// omega_c*tau_c, f = g_c*g_c, gp = g_c/(1 + g_c) and a = (3*(gp*mu))/2; an element whose tau is 0
// takes the clear line (x = 0: the identity), as in the flux kernels.  The level's six knot values
// per column are loaded together ahead of its arithmetic.  Without kSpectral nothing of this is
// read or compiled.
#pragma once

#include <hip/hip_runtime.h>

#include "path.h"
#include "radiance.h"
#include "twostream_thermal.h"

namespace lbl {

constexpr int kThermalViewAhead = 1;    // rows of beta in flight per lane

// lbl_path_thermal_radiance's: PathThermal's table, D and surface (work, level_out, top_out and
// edge are not used), with the view, the flux rows and the outputs.
struct PathThermalView : PathThermal
{
    const double * mu;          // [paths of the run]: the viewing zenith cosine
    const double * up;          // [count][stride]: up at the interface below each level
    const double * down;        // [count][stride]: down there
    double * rad;               // [paths][stride]: I at interface 0, or null
    double * bt;                // [paths][stride]: its brightness temperature, or null
};

// lbl_path_thermal_radiance_spectral's: PathThermalSpectral's table and knots with the same view,
// flux rows and outputs.
struct PathThermalViewSpectral : PathThermalSpectral
{
    const double * mu;
    const double * up;
    const double * down;
    double * rad;
    double * bt;
};

template <bool kSpectral>
using ThermalViewArguments = std::conditional_t<kSpectral, PathThermalViewSpectral, PathThermalView>;

// phi(z) = -expm1(-z)/z for z > 0, 1 at z = 0.
__device__ __forceinline__ double thermal_view_phi(double z)
{
    return z > 0. ? -expm1(-z)/z : 1.;
}

// I at the space-side face of a cloudy level from `rad` at its surface-side face (the formulas in
// the head of this file).  v: the level's scalars; d: the diffusivity factor; mu, a: the view's;
// b: beta; planck_b, pib: B(T_l) and piB(T_l); up1, down0: the fluxes at the level's surface-side
// and space-side interfaces.
__device__ __forceinline__ double thermal_view_cloudy(const ThermalLevel & v, double d, double mu,
                                                      double a, double b, double planck_b,
                                                      double pib, double up1, double down0,
                                                      double rad)
{
    const double tau_a = v.s*b;
    const double tau = tau_a + v.tau_c;
    const double omega = v.w_c/tau;
    const double sc = 1. - omega*v.f;
    const double t = sc*tau;
    const double w = ((1. - v.f)*omega)/sc;
    const double g2 = (d*(w*(1. - v.gp)))/2.;
    const double dif = d*(1. - w);
    const double g1 = g2 + dif;
    const double su = g1 + g2;
    const double k2 = dif*su;
    const double u1 = up1 - pib;
    const double d0 = down0 - pib;
    const double z = t/mu;
    const double dm = exp(-z);
    const double em = -expm1(-z);
    double c;
    if (k2*(1. + t*t) <= kThermalConservative)
    {
        const double x = g1*t;
        const double n = (u1 - d0)/(1. + x);
        const double big_w = z*(em - linear_weight(z, em));
        c = ((u1 + d0) - x*n + a*n)*em + (2.*(g1*n))*(mu*big_w);
    }
    else
    {
        const double k = sqrt(k2);
        const double e = exp(-(k*t));
        const double gamma = g2/(g1 + k);
        const double ge = gamma*e;
        const double n = 1. - ge*ge;
        const double p = (u1 - ge*d0)/n;
        const double q = (d0 - ge*u1)/n;
        const double y = ((1. - k*mu)*t)/mu;
        const double h = y >= 0. ? e*(z*thermal_view_phi(y)) : dm*(z*thermal_view_phi(-y));
        c = p*((1. + a) + gamma*(1. - a))*h +
            q*(gamma*(1. + a) + (1. - a))*((1. - e*dm)/(1. + k*mu));
    }
    return rad*dm + planck_b*em + (w/(2.*kFluxPi))*c;
}

// grid and kVector as for path_sweep_kernel; a.from_last is the order of this sweep, surface to
// space.  Whole paths: every lane starts and finishes its path.  kSpectral: the scatterer comes
// from its knot table (scatterer.h) in place of the level rows; without it nothing of that is read.
template <bool kVector, bool kSpectral = false>
__global__ __launch_bounds__(kPathThreads) void thermal_view_kernel(
    ThermalViewArguments<kSpectral> a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const int width = l.width;
    const ThermalColumns c = thermal_columns<kVector>(a, l);
    const double * level = a.level + (long long)l.index0*kThermalLevelWords;
    const double d = a.diffusivity;
    const double mu = a.mu[l.p - a.table_path];
    const long long row = (long long)l.p*a.stride + l.j;

    // The surface: what it emits, and what it reflects of the flux that reaches it -- the down
    // row of the first level of the sweep.
    double rad[kPathWidth];
    {
        double eps[kPathWidth], down[kPathWidth];
        if (a.emissivity_rows != nullptr)
        {
            path_load<kVector>(a.emissivity_rows + row, width, eps);
        }
        else
        {
            const double scalar = a.surface_e[l.p - a.table_path];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i) eps[i] = scalar;
        }
        path_load<kVector>(a.down + l.level0, width, down);
        const double ts = a.surface_t[l.p - a.table_path];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            rad[i] = eps[i]*planck(c.nu[i], c.c1nu3[i], c.c2nu[i], ts) +
                     (1. - eps[i])*(down[i]/kFluxPi);
        }
    }

    ScattererLane knots;
    if constexpr (kSpectral) knots = scatterer_lane(a.scatterer, c.nu);

    path_levels<kThermalViewAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth],
                                                        long long at) {
        if constexpr (kSpectral)
        {
            const int index = l.index0 + k*l.direction;
            ThermalLevel v = thermal_level(level + (long long)(k*l.direction)*kThermalLevelWords);
            const int m = a.scatterer.n_knots;
            const double * rows = scatterer_rows(a.scatterer, index);
            if (a.scatters[index] == 0.)
            {
#pragma unroll
                for (int i = 0; i < kPathWidth; ++i)
                {
                    const double tau_c = scatterer_value(rows, knots.j[i], knots.u[i]);
                    const double tau_a = v.s*b[i];
                    const double tau = tau_a + tau_c;
                    const double x = tau/mu;
                    rad[i] = rad[i]*exp(-x) +
                             planck(c.nu[i], c.c1nu3[i], c.c2nu[i], v.temperature)*(-expm1(-x));
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
            double up1[kPathWidth], down0[kPathWidth];
            path_load<kVector>(a.up + at, width, up1);
            if (k + 1 < l.n)
            {
                path_load<kVector>(a.down + (at + l.row_step), width, down0);
            }
            else
            {
#pragma unroll
                for (int i = 0; i < kPathWidth; ++i) down0[i] = 0.;
            }
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                v.tau_c = tau_c[i];
                // tau == 0, where the cloudy line would form 0/0: the clear line at x = 0, which
                // is rad*1 + B*0, the identity.
                if (v.s*b[i] + v.tau_c == 0.) continue;
                const double planck_b = planck(c.nu[i], c.c1nu3[i], c.c2nu[i], v.temperature);
                v.w_c = omega_c[i]*tau_c[i];
                v.f = g_c[i]*g_c[i];
                v.gp = g_c[i]/(1. + g_c[i]);
                const double view_a = (3.*(v.gp*mu))/2.;
                rad[i] = thermal_view_cloudy(v, d, mu, view_a, b[i], planck_b,
                                             thermal_pi_planck(c, i, v.temperature), up1[i],
                                             down0[i], rad[i]);
            }
            return;
        }
        const ThermalLevel v = thermal_level(level + (long long)(k*l.direction)*kThermalLevelWords);
        if (v.clear)
        {
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double tau_a = v.s*b[i];
                const double tau = tau_a + v.tau_c;
                const double x = tau/mu;
                rad[i] = rad[i]*exp(-x) +
                         planck(c.nu[i], c.c1nu3[i], c.c2nu[i], v.temperature)*(-expm1(-x));
            }
            return;
        }
        // Below this level: its own rows; above it: the next level's, or space.
        double up1[kPathWidth], down0[kPathWidth];
        path_load<kVector>(a.up + at, width, up1);
        if (k + 1 < l.n)
        {
            path_load<kVector>(a.down + (at + l.row_step), width, down0);
        }
        else
        {
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i) down0[i] = 0.;
        }
        const double view_a = (3.*(v.gp*mu))/2.;
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            const double planck_b = planck(c.nu[i], c.c1nu3[i], c.c2nu[i], v.temperature);
            rad[i] = thermal_view_cloudy(v, d, mu, view_a, b[i], planck_b,
                                         thermal_pi_planck(c, i, v.temperature), up1[i],
                                         down0[i], rad[i]);
        }
    });

    radiance_store<kVector>(a.rad, a.bt, row, width, rad, c.nu, c.c1nu3, c.c2nu);
}

}  // namespace lbl
