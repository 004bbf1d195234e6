// The lower boundary of Spectroscopy.compute_radiance (lbl_surface_emissivity,
// lbl_path_radiance_surface): a spectral emissivity per path, interpolated from a table of knots
// onto the grid, and the start value of a path whose surface also reflects.
//
//   knots k_0 < ... < k_{M-1} [cm-1], values e_0 .. e_{M-1} of a path, nu a grid point:
//   for k_j <= nu < k_{j+1}:  E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j)),
//   E = e_0 for nu <= k_0,  E = e_{M-1} for nu >= k_{M-1}
//   (numpy.interp: constant outside the knots, linear inside; each operation rounded as written,
//   so a flat table e_j = c gives E = c exactly);
//   start of a path behind a boundary at T_b whose surface reflects the radiance D that arrives
//   there:  I = E*B(nu, T_b) + (1. - E)*D, then lbl_path_radiance's update level by level.
// The TU builds with -ffp-contract=off: every product and sum is rounded as written.
//
// surface_emissivity_kernel: grid (columns / (kPathThreads*kPathWidth), paths), path_lane's
// placement -- a lane has kPathWidth consecutive columns of one path.  The M knots and the path's M
// values are staged in LDS (16 KiB at M = 1024).  On an ascending grid the 128 columns of a
// wavefront usually lie in one knot interval: the wavefront searches its first and its last column
// once, and where they agree every lane uses that interval; otherwise, and on a grid that is not
// ascending, every lane searches its own columns in LDS.  The kernel writes 8 bytes per point and
// path and reads the grid: it is bound by HBM.
#pragma once

#include <hip/hip_runtime.h>

#include "path.h"

namespace lbl {

constexpr int kSurfaceMaxKnots = 1024;

struct SurfaceEmissivity
{
    const double * nu;          // [columns]: the grid [cm-1]
    long long columns;
    long long stride;           // row stride of `rows` [values]
    const double * knot;        // [n_knots]: the knots [cm-1], strictly ascending
    const double * value;       // [paths of the launch][n_knots]: each path's emissivities
    int n_knots;
    int ascending;              // the grid does not decrease: a wavefront may share its search
    double * rows;              // row of blockIdx.y == 0
};

// The number of knots <= nu, less one: j in 0 .. M-2 for k_j <= nu < k_{j+1}, M-1 for
// nu >= k_{M-1}, and -1 for nu <= k_0 (E = e_0 there, on the knot too) and for NaN.
__device__ __forceinline__ int surface_interval(const double * knot, int m, double nu)
{
    if (!(nu > knot[0])) return -1;
    int lo = 1, hi = m;         // knots [0, lo) are <= nu, knots [hi, m) are > nu
    while (lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if (knot[mid] <= nu) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ double surface_value(const double * knot, const double * e, int m,
                                                int j, double nu)
{
    if (j < 0) return e[0];
    if (j >= m - 1) return e[m - 1];
    return e[j] + (nu - knot[j])*((e[j + 1] - e[j])/(knot[j + 1] - knot[j]));
}

// kVector: every row starts 16-byte aligned (even stride, aligned bases), the grid too.
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void surface_emissivity_kernel(SurfaceEmissivity a)
{
    __shared__ double knot[kSurfaceMaxKnots];
    __shared__ double value[kSurfaceMaxKnots];
    const int m = a.n_knots;
    const double * e = a.value + (long long)blockIdx.y*m;
    for (int i = (int)threadIdx.x; i < m; i += kPathThreads)
    {
        knot[i] = a.knot[i];
        value[i] = e[i];
    }
    __syncthreads();

    const long long j = ((long long)blockIdx.x*kPathThreads + threadIdx.x)*kPathWidth;
    if (j >= a.columns) return;
    const int width = (int)(a.columns - j < kPathWidth ? a.columns - j : kPathWidth);
    double nu[kPathWidth];
    path_load<kVector>(a.nu + j, width, nu);

    // The wavefront's first and last column (the first lies inside the grid: this lane does).
    bool shared = false;
    int interval = 0;
    if (a.ascending)
    {
        const long long first = ((long long)blockIdx.x*kPathThreads + (threadIdx.x & ~63u))*kPathWidth;
        const long long end = first + 64*kPathWidth < a.columns ? first + 64*kPathWidth : a.columns;
        const int lo = surface_interval(knot, m, a.nu[first]);
        const int hi = surface_interval(knot, m, a.nu[end - 1]);
        shared = lo == hi;
        interval = __builtin_amdgcn_readfirstlane(lo);
    }
    double out[kPathWidth];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        const int at = shared ? interval : surface_interval(knot, m, nu[i]);
        out[i] = surface_value(knot, value, m, at, nu[i]);
    }
    path_store<kVector>(a.rows + (long long)blockIdx.y*a.stride + j, width, out);
}

}  // namespace lbl
