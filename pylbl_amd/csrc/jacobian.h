// Analytic radiance Jacobians along paths (Spectroscopy.compute_jacobian, lbl_path_jacobian): the
// derivatives of radiance.h's isothermal-layer recurrence with respect to the state of every
// level, from what a radiance call already has in HBM.
//
// For one path and one grid point, the levels numbered k = 0 .. L-1 in sweep order, with
// x_k = s_k*beta_k, t_k = exp(-x_k), a_k = -expm1(-x_k), B_k = B(nu, T_k) (radiance.h):
//   forward:   I_-1 = eps*B(nu, T_b) (or 0),  I_k = I_{k-1}*t_k + B_k*a_k,  radiance = I_{L-1}
//   trailing:  tau'_{L-1} = 0,  tau'_{k-1} = tau'_k + s_k*beta_k  (summed from the observer
//              backwards),  trail_k = exp(-tau'_k),  trail_b = exp(-tau'_{-1})
//   dB(nu, T) = (B*(u/T))*(1. + B/(((C1*nu)*nu)*nu)),  u = (C2*nu)/T,  0 for nu <= 0
//   dI/dx_k    = (B_k - I_k)*trail_k            (B_k - I_k = (B_k - I_{k-1})*t_k)
//   dI/dln x_k = x_k*((B_k - I_k)*trail_k)
//   dI/dT_k    = (a_k*dB(nu, T_k))*trail_k      (at fixed beta: the source function alone)
//   dI/dT_b    = (eps*dB(nu, T_b))*trail_b,     dI/deps = B(nu, T_b)*trail_b
// The TU builds with -ffp-contract=off: every product and sum is rounded as written.
//
// path_jacobian_kernel runs whole paths on path.h's sweep skeleton, in two loops by the same lane
// over the same columns.  Loop 1 goes against the sweep order (the lane of the opposite
// direction, from the same PathLevels) with kPathAhead rows of beta in flight, like
// path_sweep_kernel: it writes trail_k into the level's row of the work block W before it adds
// the level, and ends with tau'_{-1}, from which the boundary Jacobians are formed.  Loop 2 is
// path_radiance_kernel's update in sweep order with kJacobianAhead rows of beta and of W in
// flight, and forms the requested Jacobians of a level from I_k, B_k, x_k and W's row.  An output
// may be W itself: the lane that reads an element is the one that writes it, after reading it.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lbl_amd.h"
#include "path.h"
#include "radiance.h"

namespace lbl {

// Rows of beta and of W in flight per lane in loop 2: together the kPathAhead 16-byte loads of
// the radiance kernel, whose registers this kernel's loop 2 needs as well.
constexpr int kJacobianAhead = 4;

struct PathJacobian : PathLevels       // (carry is not used: a launch holds whole paths)
{
    const double * nu;          // [columns]: the grid [cm-1]
    const double * length;      // [count]: path length of flat level first + i [m]
    const double * temperature; // [count]: temperature of flat level first + i [K]
    const double * boundary_t;  // [paths of the run]: boundary temperature, 0 = none [K]
    const double * boundary_e;  // [paths of the run]: boundary emissivity
    int table_path;             // path of boundary_t[0] / boundary_e[0]
    double * work;              // W: row r is trail of flat level row_base + r; rows `stride` apart
    double * d_depth;           // per level, laid out like W (may be W): dI/dx, or null
    double * d_log_depth;       // per level (may be W): dI/dln x, or null
    double * d_temperature;     // per level: dI/dT, or null
    double * radiance;          // [paths][stride]: I of the path, or null
    double * d_boundary_t;      // [paths][stride]: dI/dT_b, or null
    double * d_boundary_e;      // [paths][stride]: dI/deps, or null
};

// dB/dT of radiance.h's planck(), from its value b.
__device__ __forceinline__ double planck_dt(double nu, double c1nu3, double c2nu, double t,
                                            double b)
{
    return nu > 0. ? (b*((c2nu/t)/t))*(1. + b/c1nu3) : 0.;
}

// path_levels with a second row stream `other`, laid out like beta: step(k, b, w, at).
template <int kAhead, bool kVector, typename Step>
__device__ __forceinline__ void path_levels_pair(const PathLevels & a, const PathLane & l,
                                                 const double * other, Step step)
{
    const double * beta = a.beta + l.level0;
    other += l.level0;
    int k = 0;
    for (; k + kAhead <= l.n; k += kAhead)
    {
        double b[kAhead][kPathWidth], w[kAhead][kPathWidth];
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
        {
            path_load<kVector>(beta + (long long)(k + u)*l.row_step, l.width, b[u]);
            path_load<kVector>(other + (long long)(k + u)*l.row_step, l.width, w[u]);
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
        {
            step(k + u, b[u], w[u], l.level0 + (long long)(k + u)*l.row_step);
        }
    }
    for (; k < l.n; ++k)
    {
        double b[kPathWidth], w[kPathWidth];
        path_load<kVector>(beta + (long long)k*l.row_step, l.width, b);
        path_load<kVector>(other + (long long)k*l.row_step, l.width, w);
        step(k, b, w, l.level0 + (long long)k*l.row_step);
    }
}

// grid and kVector as for path_sweep_kernel; [first, first + count) holds whole paths.
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void path_jacobian_kernel(PathJacobian a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const int width = l.width;
    const long long row = (long long)l.p*a.stride + l.j;

    double nu[kPathWidth], c1nu3[kPathWidth], c2nu[kPathWidth];
    path_load<kVector>(a.nu + l.j, width, nu);
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        c1nu3[i] = ((LBL_PLANCK_C1*nu[i])*nu[i])*nu[i];
        c2nu[i] = LBL_PLANCK_C2*nu[i];
    }
    const double tb = a.boundary_t[l.p - a.table_path];
    const double eb = a.boundary_e[l.p - a.table_path];

    // Loop 1, from the observer backwards: trail_k into W, then tau' = tau' + s_k*beta_k.
    {
        PathLevels against = a;
        against.from_last = !a.from_last;
        const PathLane r = path_lane(against);
        const double * length = a.length + r.index0;
        double tau[kPathWidth];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) tau[i] = 0.;
        path_levels<kPathAhead, kVector>(against, r,
                                         [&](int k, const double (&b)[kPathWidth], long long at) {
            path_store_exp<kVector>(a.work + at, width, tau);
            const double s = length[k*r.direction];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i) tau[i] = tau[i] + s*b[i];
        });
        if (a.d_boundary_t != nullptr || a.d_boundary_e != nullptr)
        {
            double dt[kPathWidth], de[kPathWidth];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double trail = exp(-tau[i]);
                const double b = tb > 0. ? planck(nu[i], c1nu3[i], c2nu[i], tb) : 0.;
                dt[i] = tb > 0. ? (eb*planck_dt(nu[i], c1nu3[i], c2nu[i], tb, b))*trail : 0.;
                de[i] = b*trail;
            }
            if (a.d_boundary_t != nullptr) path_store<kVector>(a.d_boundary_t + row, width, dt);
            if (a.d_boundary_e != nullptr) path_store<kVector>(a.d_boundary_e + row, width, de);
        }
    }

    // Loop 2, in sweep order: the radiance update, then the level's Jacobians.
    const double * length = a.length + l.index0;
    const double * temperature = a.temperature + l.index0;
    double rad[kPathWidth];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        rad[i] = tb > 0. ? eb*planck(nu[i], c1nu3[i], c2nu[i], tb) : 0.;
    }
    path_levels_pair<kJacobianAhead, kVector>(
        a, l, a.work, [&](int k, const double (&b)[kPathWidth], const double (&w)[kPathWidth],
                          long long at) {
        const double s = length[k*l.direction];
        const double t = temperature[k*l.direction];
        double dx[kPathWidth], dlog[kPathWidth], dt[kPathWidth];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            const double x = s*b[i];
            const double source = planck(nu[i], c1nu3[i], c2nu[i], t);
            const double emitted = -expm1(-x);
            rad[i] = rad[i]*exp(-x) + source*emitted;
            dx[i] = (source - rad[i])*w[i];
            dlog[i] = x*dx[i];
            if (a.d_temperature != nullptr)
            {
                dt[i] = (emitted*planck_dt(nu[i], c1nu3[i], c2nu[i], t, source))*w[i];
            }
        }
        if (a.d_depth != nullptr) path_store<kVector>(a.d_depth + at, width, dx);
        if (a.d_log_depth != nullptr) path_store<kVector>(a.d_log_depth + at, width, dlog);
        if (a.d_temperature != nullptr) path_store<kVector>(a.d_temperature + at, width, dt);
    });
    if (a.radiance != nullptr) path_store<kVector>(a.radiance + row, width, rad);
}

}  // namespace lbl
