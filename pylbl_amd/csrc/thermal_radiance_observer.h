// Radiances through clouds at an observer inside, above or below the atmosphere, looking down or
// up (Spectroscopy.compute_thermal_radiance_at, lbl_path_thermal_radiance_observer): the view
// sweeps of thermal_radiance.h and thermal_radiance_source.h, run in either direction and stopped
// after the levels the ray passes.  The TU builds with -ffp-contract=off: every product, sum and
// quotient is rounded as written.
//
// Inputs.  thermal_radiance.h's, bit for bit: the level row, D, mu, the flux rows up[i], down[i] at
// interface i (interface 0 faces space, level i lies between interfaces i and i + 1), and with an
// edge table thermal_radiance_source.h's interface temperatures.  n_p in [0, L]: the levels the ray
// of path p passes.
// Model.  A ray that travels downward through a level is the ray that travels upward through the
// mirrored level, and the layer's two-stream solution is symmetric under that mirror (f+ and f-,
// the two faces and the sign of the source's slope change places).  So with E the face by which
// the ray enters a level and X the face by which it leaves, F_with the flux travelling with the
// ray at E, F_against the flux travelling against it at X, and B_E, B_X the Planck values at the
// two faces, the level maps I_E to I_X by the existing lines with
//   up1 := F_with ; down0 := F_against ; bb := B_E ; bt := B_X ; a = (3*(gp*mu))/2
// in thermal_view_cloudy, thermal_view_kernel's clear line, thermal_view_cloudy_source and
// linear_update.
//   looking down: E is the surface-side face; F_with = up[i+1] ; F_against = down[i]
//     start: the surface line I = eps*B(T_s) + (1 - eps)*(down[L]/pi)
//     the n_p levels nearest the surface, in order; the result is I at interface L - n_p
//   looking up: E is the space-side face; F_with = down[i] ; F_against = up[i+1]
//     start: I = 0 at interface 0
//     levels 0 ... n_p - 1 counted from space; the result is I at interface n_p
//     with the edge table:  c = (pi*(B_space - B_surface))/(su*t)
//       u1 = (down[i] - pi*B_space) - c ; d0 = (up[i+1] - pi*B_surface) + c
// down[0] = 0 is the constant at the path's space end only and is used where level 0 itself is
// passed; an observer inside the atmosphere has a real down row at its interface, which is read.
// With n_p = L, looking down is thermal_view_kernel (thermal_view_source_kernel with the edge
// table) bit for bit.  n_p = 0 writes the start value.
//
// thermal_observer_kernel runs on path.h's sweep skeleton with the lane's step count cut to n_p.
// blockIdx.y is the path, so n_p, mu, the direction and the level row are the same for the whole
// wavefront.  The flux rows hold up and down at the interface on the surface side of each level:
// looking down, F_with is the step's own up row and F_against the down row of the next step (0 at
// the path's last level); looking up, F_with is the down row of the previous step (0 at step 0)
// and F_against the step's own up row.  A clear level reads no flux row.  kLinear: a lane
// evaluates Planck once at the face it enters its path by and once per level at the face it leaves
// by, which it keeps for the next level, as thermal_view_source_kernel does.  The kernels of
// thermal_radiance.h and thermal_radiance_source.h are not touched.
#pragma once

#include <hip/hip_runtime.h>

#include "path.h"
#include "radiance.h"
#include "thermal_radiance.h"
#include "thermal_radiance_source.h"
#include "twostream_thermal.h"

namespace lbl {

constexpr int kThermalObserverAhead = 1;    // rows of beta in flight per lane, as the two view sweeps

// lbl_path_thermal_radiance_observer's: PathThermalView's (edge: null without the linear source)
// with the levels every ray passes.
struct PathThermalObserver : PathThermalView
{
    const double * observer;    // [paths of the run]: n_p, a whole number in [0, levels_per_path]
};

// grid and kVector as for path_sweep_kernel; a.from_last is the order of this sweep: surface to
// space looking down, space to surface with kUp.  Whole paths in the launch; a lane takes the
// first n_p levels of its path in that order.
template <bool kVector, bool kLinear, bool kUp>
__global__ __launch_bounds__(kPathThreads) void thermal_observer_kernel(PathThermalObserver a)
{
    PathLane l = path_lane(a);
    if (l.idle) return;
    const int whole = l.n;
    l.n = (int)a.observer[l.p - a.table_path];
    const int width = l.width;
    const ThermalColumns c = thermal_columns<kVector>(a, l);
    const double * level = a.level + (long long)l.index0*kThermalLevelWords;
    const double d = a.diffusivity;
    const double mu = a.mu[l.p - a.table_path];
    const long long row = (long long)l.p*a.stride + l.j;

    double rad[kPathWidth];
    if constexpr (kUp)
    {
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) rad[i] = 0.;
    }
    else
    {
        // The surface, as in thermal_view_kernel.
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

    // kLinear: Planck at the face the lane enters its first level by.
    const int side = entry_side(l.direction);
    const double * edge = kLinear ? a.edge + 2*(long long)l.index0 : nullptr;
    double be[kPathWidth];
    if constexpr (kLinear)
    {
        const double t = edge[side];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) be[i] = planck(c.nu[i], c.c1nu3[i], c.c2nu[i], t);
    }

    path_levels<kThermalObserverAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth],
                                                           long long at) {
        const ThermalLevel v = thermal_level(level + (long long)(k*l.direction)*kThermalLevelWords);
        double t_leave = 0.;
        if constexpr (kLinear) t_leave = edge[2*(long long)(k*l.direction) + (1 - side)];
        if (v.clear)
        {
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double tau_a = v.s*b[i];
                const double tau = tau_a + v.tau_c;
                if constexpr (kLinear)
                {
                    const double bx = planck(c.nu[i], c.c1nu3[i], c.c2nu[i], t_leave);
                    rad[i] = linear_update(rad[i], tau/mu, be[i], bx);
                    be[i] = bx;
                }
                else
                {
                    const double x = tau/mu;
                    rad[i] = rad[i]*exp(-x) +
                             planck(c.nu[i], c.c1nu3[i], c.c2nu[i], v.temperature)*(-expm1(-x));
                }
            }
            return;
        }
        // F_with at the face of entry, F_against at the face of exit.
        double with[kPathWidth], against[kPathWidth];
        if constexpr (kUp)
        {
            path_load<kVector>(a.up + at, width, against);
            if (k > 0)
            {
                path_load<kVector>(a.down + (at - l.row_step), width, with);
            }
            else
            {
#pragma unroll
                for (int i = 0; i < kPathWidth; ++i) with[i] = 0.;
            }
        }
        else
        {
            path_load<kVector>(a.up + at, width, with);
            if (k + 1 < whole)
            {
                path_load<kVector>(a.down + (at + l.row_step), width, against);
            }
            else
            {
#pragma unroll
                for (int i = 0; i < kPathWidth; ++i) against[i] = 0.;
            }
        }
        const double view_a = (3.*(v.gp*mu))/2.;
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            if constexpr (kLinear)
            {
                const double bx = planck(c.nu[i], c.c1nu3[i], c.c2nu[i], t_leave);
                rad[i] = thermal_view_cloudy_source(v, d, mu, view_a, b[i], bx, be[i], with[i],
                                                    against[i], rad[i]);
                be[i] = bx;
            }
            else
            {
                const double planck_b = planck(c.nu[i], c.c1nu3[i], c.c2nu[i], v.temperature);
                rad[i] = thermal_view_cloudy(v, d, mu, view_a, b[i], planck_b,
                                             thermal_pi_planck(c, i, v.temperature), with[i],
                                             against[i], rad[i]);
            }
        }
    });

    radiance_store<kVector>(a.rad, a.bt, row, width, rad, c.nu, c.c1nu3, c.c2nu);
}

}  // namespace lbl
