// Sounder radiances through clouds with a source that is linear in optical depth
// (Spectroscopy.compute_thermal_radiance_linear, lbl_path_thermal_radiance_source): the view sweep
// of thermal_radiance.h with the Planck function of every level running linearly in its
// delta-scaled optical depth between the values at the level's two interfaces, from the fluxes
// lbl_path_thermal_two_stream_source (twostream_thermal.h, kLinear) wrote from the same edge table.
// The TU builds with -ffp-contract=off: every product, sum and quotient below is rounded as
// written.
//
// Inputs.  thermal_radiance.h's, bit for bit: the level row, D, mu, tau, the clear/cloudy
// wave-uniform branch, omega, sc, t, w, g2, dif, g1, su, k2, the conservative criterion, k, E,
// Gamma, gp, a, Dm, Em, h, W, the surface line and the result at interface 0.  T_l sets beta only.
// edge [count][2]: the interface temperatures of each flat level, read as PathThermal::edge is.
//   Bt = planck(T at the level's space-side interface) ; Bb = planck(T at its surface-side one)
//   dB = Bb - Bt
// Model.  B(tau) = Bt + dB*tau/t for tau in [0, t] from the space-side face.  The two-stream
// system with this source has the particular solution F+-p = pi*(B(tau) +- B'/su), so with
//   c = (pi*dB)/(su*t)
// f+ = [thermal_radiance.h's homogeneous part] + c and f- = [the same] - c, and
//   u1 = (up[i+1] - pi*Bb) - c ; d0 = (down[i] - pi*Bt) + c      (P, Q, N from these, as there)
//   C = [thermal_radiance.h's C of its branch, general or conservative] + (2*(a*c))*Em
// cloudy:
//   I_top = I_bot*Dm + (Bt*Em + dB*(Em - linear_weight(t/mu, Em))) + (w/(2 pi))*C
// clear (w_c == 0, the same for the whole wavefront; radiance.h's linear_update):
//   x = tau/mu ; A = -expm1(-x) ; lw = linear_weight(x, A)
//   I_top = I_bot*exp(-x) + (Bb*(A - lw) + Bt*lw)
// su = D*(1 - w*gp) >= D/2 bounds c by 2*pi*dB/(D*t); it enters the radiance multiplied by about
// t/mu, so the sum stays well conditioned in a thin level.  With dB = 0 the cloudy line is
// thermal_radiance.h's to the bit (c = 0, `+ 0`); the clear line is path_radiance_kernel's
// linear one: mu = 1 without tau_c gives its bits.
//
// thermal_view_source_kernel is thermal_view_kernel's sweep, surface -> space with I in registers,
// whole paths only.  A lane evaluates Planck once at the face by which it enters its path and once
// per level at the face it leaves the level by, which it keeps as the next level's entry value
// (Bb), as path_radiance_kernel and ThermalFaces do.  A clear level reads no flux row.  It is a
// kernel of its own, so that thermal_view_kernel's instantiations keep their instructions.
#pragma once

#include <hip/hip_runtime.h>

#include "path.h"
#include "radiance.h"
#include "thermal_radiance.h"
#include "twostream_thermal.h"

namespace lbl {

constexpr int kThermalViewSourceAhead = 1;  // rows of beta in flight per lane

// thermal_view_cloudy with the linear source (the formulas in the head of this file).  bt, bb:
// planck at the level's space-side and surface-side interfaces.
__device__ __forceinline__ double thermal_view_cloudy_source(const ThermalLevel & v, double d,
                                                             double mu, double a, double b,
                                                             double bt, double bb, double up1,
                                                             double down0, double rad)
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
    const double db = bb - bt;
    const double cs = (kFluxPi*db)/(su*t);
    const double u1 = (up1 - kFluxPi*bb) - cs;
    const double d0 = (down0 - kFluxPi*bt) + cs;
    const double z = t/mu;
    const double dm = exp(-z);
    const double em = -expm1(-z);
    const double lw = linear_weight(z, em);
    double c;
    if (k2*(1. + t*t) <= kThermalConservative)
    {
        const double x = g1*t;
        const double n = (u1 - d0)/(1. + x);
        const double big_w = z*(em - lw);
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
    c = c + (2.*(a*cs))*em;
    return rad*dm + (bt*em + db*(em - lw)) + (w/(2.*kFluxPi))*c;
}

// grid and kVector as for path_sweep_kernel; a.from_last is the order of this sweep, surface to
// space: a level is entered through its surface-side face (Bb) and left through the other (Bt).
// Whole paths: every lane starts and finishes its path.  a.edge must not be null.
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void thermal_view_source_kernel(PathThermalView a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const int width = l.width;
    const ThermalColumns c = thermal_columns<kVector>(a, l);
    const double * level = a.level + (long long)l.index0*kThermalLevelWords;
    const double d = a.diffusivity;
    const double mu = a.mu[l.p - a.table_path];
    const long long row = (long long)l.p*a.stride + l.j;

    // The surface, as in thermal_view_kernel: T_s stays apart from the interface's temperature.
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

    // Planck at the face the lane enters its first level by: the surface-side one.
    const int side = entry_side(l.direction);
    const double * edge = a.edge + 2*(long long)l.index0;
    double bb[kPathWidth];
    {
        const double t = edge[side];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) bb[i] = planck(c.nu[i], c.c1nu3[i], c.c2nu[i], t);
    }

    path_levels<kThermalViewSourceAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth],
                                                              long long at) {
        const ThermalLevel v = thermal_level(level + (long long)(k*l.direction)*kThermalLevelWords);
        const double t_leave = edge[2*(long long)(k*l.direction) + (1 - side)];
        if (v.clear)
        {
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double tau_a = v.s*b[i];
                const double tau = tau_a + v.tau_c;
                const double bt = planck(c.nu[i], c.c1nu3[i], c.c2nu[i], t_leave);
                rad[i] = linear_update(rad[i], tau/mu, bb[i], bt);
                bb[i] = bt;
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
            const double bt = planck(c.nu[i], c.c1nu3[i], c.c2nu[i], t_leave);
            rad[i] = thermal_view_cloudy_source(v, d, mu, view_a, b[i], bt, bb[i], up1[i],
                                                down0[i], rad[i]);
            bb[i] = bt;
        }
    });

    radiance_store<kVector>(a.rad, a.bt, row, width, rad, c.nu, c.c1nu3, c.c2nu);
}

}  // namespace lbl
