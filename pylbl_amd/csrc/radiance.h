// Thermal emission along paths (Spectroscopy.compute_radiance, lbl_path_radiance): the
// Schwarzschild sweep over the "total" absorption block in HBM, with isothermal layers.
//
//   B(nu, T) = (((C1*nu)*nu)*nu) / expm1((C2*nu)/T), 0 for nu <= 0  [W m-2 sr-1 (cm-1)-1]
//   layer of level l, x = s_l*beta_l:  t = exp(-x),  a = -expm1(-x),  source B(nu, T_l)
//   I = eps*B(nu, T_boundary) (or 0), then I = I*t + B_l*a level by level in sweep order.
//   brightness temperature = (C2*nu) / log1p((((C1*nu)*nu)*nu) / I), 0 where I <= 0 or nu <= 0.
// The TU builds with -ffp-contract=off: every product and sum is rounded as written.
//
// path_radiance_kernel is path_sweep_kernel (path.h) with the radiance update in place of
// tau = tau + s*beta: a lane owns kPathWidth consecutive columns, has kPathAhead rows in flight,
// keeps I in registers and forms nu, C2*nu and ((C1*nu)*nu)*nu once.  s_l and T_l are the same for
// the whole wavefront.  Per element: two divisions (Planck's argument and Planck itself), one
// expm1 for Planck, one exp and one expm1 for the layer, the update -- fp64 VALU work of the same
// order as the HBM time of reading the row.  Band means go through path.h's band kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lbl_amd.h"
#include "path.h"

namespace lbl {

struct PathRadiance
{
    const double * beta;        // row of flat level `row_base`; rows `stride` apart
    long long stride;           // row stride of beta, carry, level and final outputs [values]
    long long columns;
    const double * nu;          // [columns]: the grid [cm-1]
    const double * length;      // [count]: path length of flat level first + i [m]
    const double * temperature; // [count]: temperature of flat level first + i [K]
    const double * boundary_t;  // [paths of the run]: boundary temperature, 0 = none [K]
    const double * boundary_e;  // [paths of the run]: boundary emissivity
    int first, count;           // the flat levels of this launch
    int row_base;               // flat level of row 0 of beta and the level outputs
    int levels_per_path;
    int first_path;             // path of blockIdx.y == 0
    int table_path;             // path of boundary_t[0] / boundary_e[0]
    int from_last;              // sweep each path from its last level down
    double * carry;             // [paths][stride]: I of a path between runs
    double * level_rad;         // cumulative: I after each level (may be beta itself), or null
    double * level_bt;          // cumulative: brightness temperature after each level, or null
    double * final_rad;         // [paths][stride]: I of a finished path, or null
    double * final_bt;          // [paths][stride]: its brightness temperature, or null
    int keep_final;             // a finished path's I stays in its carry row (band means)
};

__device__ __forceinline__ double planck(double nu, double c1nu3, double c2nu, double t)
{
    return nu > 0. ? c1nu3/expm1(c2nu/t) : 0.;
}

__device__ __forceinline__ double brightness(double nu, double c1nu3, double c2nu, double i)
{
    return nu > 0. && i > 0. ? c2nu/log1p(c1nu3/i) : 0.;
}

// Writes I and/or its brightness temperature at offset `at` of the chosen outputs.
template <bool kVector>
__device__ __forceinline__ void radiance_store(double * rad, double * bt, long long at, int width,
                                               const double (&i_)[kPathWidth],
                                               const double (&nu)[kPathWidth],
                                               const double (&c1nu3)[kPathWidth],
                                               const double (&c2nu)[kPathWidth])
{
    if (rad != nullptr) path_store<kVector>(rad + at, width, i_);
    if (bt != nullptr)
    {
        double t[kPathWidth];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) t[i] = brightness(nu[i], c1nu3[i], c2nu[i], i_[i]);
        path_store<kVector>(bt + at, width, t);
    }
}

// grid (columns / (kPathThreads*kPathWidth), paths touched by [first, first + count)).
// kVector: every row starts 16-byte aligned (even stride, aligned bases).
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void path_radiance_kernel(PathRadiance a)
{
    const long long j = ((long long)blockIdx.x*kPathThreads + threadIdx.x)*kPathWidth;
    if (j >= a.columns) return;
    const int width = (int)(a.columns - j < kPathWidth ? a.columns - j : kPathWidth);
    const int p = a.first_path + (int)blockIdx.y;
    const int path_lo = p*a.levels_per_path, path_hi = path_lo + a.levels_per_path;
    const int lo = max(a.first, path_lo), hi = min(a.first + a.count, path_hi);
    if (lo >= hi) return;
    const bool starts = a.from_last ? hi == path_hi : lo == path_lo;
    const bool finishes = a.from_last ? lo == path_lo : hi == path_hi;
    const int n = hi - lo;
    // Level of the k-th step: lo + k upward, hi - 1 - k downward.
    const int origin = a.from_last ? hi - 1 : lo;
    const int direction = a.from_last ? -1 : 1;
    const long long row_step = (long long)direction*a.stride;
    const double * beta = a.beta + (long long)(origin - a.row_base)*a.stride + j;
    const double * length = a.length + (origin - a.first);
    const double * temperature = a.temperature + (origin - a.first);

    double nu[kPathWidth], c1nu3[kPathWidth], c2nu[kPathWidth];
    path_load<kVector>(a.nu + j, width, nu);
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        c1nu3[i] = ((LBL_PLANCK_C1*nu[i])*nu[i])*nu[i];
        c2nu[i] = LBL_PLANCK_C2*nu[i];
    }

    double rad[kPathWidth];
    if (starts)
    {
        const double tb = a.boundary_t[p - a.table_path];
        const double eb = a.boundary_e[p - a.table_path];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            rad[i] = tb > 0. ? eb*planck(nu[i], c1nu3[i], c2nu[i], tb) : 0.;
        }
    }
    else
    {
        path_load<kVector>(a.carry + (long long)p*a.stride + j, width, rad);
    }
    const bool per_level = a.level_rad != nullptr || a.level_bt != nullptr;
    const long long level0 = (long long)(origin - a.row_base)*a.stride + j;

    int k = 0;
    for (; k + kPathAhead <= n; k += kPathAhead)
    {
        double b[kPathAhead][kPathWidth];
#pragma unroll
        for (int u = 0; u < kPathAhead; ++u)
        {
            path_load<kVector>(beta + (long long)(k + u)*row_step, width, b[u]);
        }
#pragma unroll
        for (int u = 0; u < kPathAhead; ++u)
        {
            const double s = length[(k + u)*direction];
            const double t = temperature[(k + u)*direction];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double x = s*b[u][i];
                rad[i] = rad[i]*exp(-x) + planck(nu[i], c1nu3[i], c2nu[i], t)*(-expm1(-x));
            }
            if (per_level)
            {
                radiance_store<kVector>(a.level_rad, a.level_bt, level0 + (long long)(k + u)*row_step,
                                        width, rad, nu, c1nu3, c2nu);
            }
        }
    }
    for (; k < n; ++k)
    {
        double b[kPathWidth];
        path_load<kVector>(beta + (long long)k*row_step, width, b);
        const double s = length[k*direction];
        const double t = temperature[k*direction];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            const double x = s*b[i];
            rad[i] = rad[i]*exp(-x) + planck(nu[i], c1nu3[i], c2nu[i], t)*(-expm1(-x));
        }
        if (per_level)
        {
            radiance_store<kVector>(a.level_rad, a.level_bt, level0 + (long long)k*row_step, width,
                                    rad, nu, c1nu3, c2nu);
        }
    }

    const long long row = (long long)p*a.stride + j;
    if (!finishes || a.keep_final) path_store<kVector>(a.carry + row, width, rad);
    if (finishes) radiance_store<kVector>(a.final_rad, a.final_bt, row, width, rad, nu, c1nu3, c2nu);
}

}  // namespace lbl
