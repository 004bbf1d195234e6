// Thermal emission along paths (Spectroscopy.compute_radiance, lbl_path_radiance): the
// Schwarzschild sweep over the "total" absorption block in HBM, with isothermal layers or, in
// the kLinear instantiations (lbl_path_radiance_source with edge temperatures), a source that is
// linear in optical depth between the Planck values at a layer's two interfaces.
//
//   B(nu, T) = (((C1*nu)*nu)*nu) / expm1((C2*nu)/T), 0 for nu <= 0  [W m-2 sr-1 (cm-1)-1]
//   layer of level l, x = s_l*beta_l:  t = exp(-x),  a = -expm1(-x),  source B(nu, T_l)
//   I = eps*B(nu, T_boundary) (or 0), then I = I*t + B_l*a level by level in sweep order.
//   brightness temperature = (C2*nu) / log1p((((C1*nu)*nu)*nu) / I), 0 where I <= 0 or nu <= 0.
// Linear-in-tau source (kLinear), B_in / B_out = B(nu, T) at the interface the sweep enters the
// level through / leaves it through:
//   w = 1 - a/x, u_in = a - w, I = I*t + (B_in*u_in + B_out*w)
//   w is formed as 1. - a/x for |x| >= 1/16 and below that as the 8-term Horner series
//     x*(1./2. - x*(1./6. - x*(1./24. - x*(1./120. - x*(1./720. - x*(1./5040. - x*(1./40320.
//       - x*(1./362880.))))))))
//   (1 - a/x is 0/0 at x = 0 and loses x's leading digits below it: 4e-4 relative at x = 1e-12;
//   the two-branch form stays within 6.2e-15 relative of long double from x = -3 to 1e3).
//   x = 0 gives w = u_in = 0 and t = 1: I is unchanged bit for bit.
// Reflecting surface and spectral emissivity (path_radiance_surface_kernel, lbl_path_radiance_surface;
// the table and its interpolation are surface.h's): a path that starts behind a boundary starts from
//   I = E*B(nu, T_boundary) + (1. - E)*D
// with E the path's emissivity at nu (or the scalar eps) and D the radiance that arrives at the
// boundary (or E*B alone where nothing is reflected).  Only the start differs: both kernels run the
// same radiance_sweep, and path_radiance_kernel's instantiations are what they were.
// The TU builds with -ffp-contract=off: every product and sum is rounded as written.
//
// path_radiance_kernel runs on path.h's sweep skeleton with kPathAhead rows in flight: a lane
// keeps I in registers and forms nu, C2*nu and ((C1*nu)*nu)*nu once.  s_l and T_l are the same for
// the whole wavefront.  Per element: two divisions (Planck's argument and Planck itself), one
// expm1 for Planck, one exp and one expm1 for the layer, the update -- fp64 VALU work of the same
// order as the HBM time of reading the row.  Band means go through path.h's band kernels.
// kLinear: the lane evaluates Planck at the entry interface of the first level it handles in the
// launch and then once per level at the exit interface, which it keeps in registers as the next
// level's B_in (the table is continuous within a path: the entry checks it) -- one Planck per
// element and level as before, plus one division and the weight.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lbl_amd.h"
#include "path.h"

namespace lbl {

struct PathRadiance : PathLevels
{
    const double * nu;          // [columns]: the grid [cm-1]
    const double * length;      // [count]: path length of flat level first + i [m]
    const double * temperature; // [count]: temperature of flat level first + i [K]
    const double * boundary_t;  // [paths of the run]: boundary temperature, 0 = none [K]
    const double * boundary_e;  // [paths of the run]: boundary emissivity
    int table_path;             // path of boundary_t[0] / boundary_e[0]
    double * level_rad;         // cumulative: I after each level (may be beta itself), or null
    double * level_bt;          // cumulative: brightness temperature after each level, or null
    double * final_rad;         // [paths][stride]: I of a finished path, or null
    double * final_bt;          // [paths][stride]: its brightness temperature, or null
    int keep_final;             // a finished path's I stays in its carry row (band means)
    const double * edge;        // [count][2]: interface temperatures of flat level first + i on
                                // its first-level / last-level side [K] (kLinear), or null
};

constexpr double kLinearSeriesBelow = 1./16.;   // |x| below which w comes from its series

// w = 1 - a/x for a = -expm1(-x): the weight of B_out in a layer of optical depth x.
__device__ __forceinline__ double linear_weight(double x, double a)
{
    const double series =
        x*(1./2. - x*(1./6. - x*(1./24. - x*(1./120. - x*(1./720. - x*(1./5040. - x*(1./40320. -
        x*(1./362880.))))))));
    return fabs(x) < kLinearSeriesBelow ? series : 1. - a/x;
}

// One level with the linear-in-tau source: I*t + (B_in*u_in + B_out*w).
__device__ __forceinline__ double linear_update(double i, double x, double b_in, double b_out)
{
    const double a = -expm1(-x);
    const double w = linear_weight(x, a);
    return i*exp(-x) + (b_in*(a - w) + b_out*w);
}

// The side ([.][0] or [.][1] of the edge table) a sweep in `direction` enters a level through.
__device__ __forceinline__ int entry_side(int direction)
{
    return direction > 0 ? 0 : 1;
}

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

// What lbl_path_radiance_surface adds to the arguments (the kSurface kernels): device rows
// [paths][stride] like the carry rows, read where a path starts.
struct PathSurface : PathRadiance
{
    const double * emissivity_rows; // E per path and column, or null: boundary_e of the path
    const double * reflection;      // D per path and column, or null: nothing is reflected
};

// The sweep of one lane.  kLinear: the linear-in-tau source of a.edge.  kSurface (Args =
// PathSurface): a path that starts in the launch behind a boundary starts from
// E*B(nu, T_boundary) + (1. - E)*D with E and D read from a.emissivity_rows and a.reflection
// (E = eps without the rows; E*B alone without D); nothing else differs.
template <bool kVector, bool kLinear, bool kSurface, typename Args>
__device__ __forceinline__ void radiance_sweep(const Args & a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const double * length = a.length + l.index0;
    const double * temperature = a.temperature + l.index0;
    const int width = l.width;

    double nu[kPathWidth], c1nu3[kPathWidth], c2nu[kPathWidth];
    path_load<kVector>(a.nu + l.j, width, nu);
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        c1nu3[i] = ((LBL_PLANCK_C1*nu[i])*nu[i])*nu[i];
        c2nu[i] = LBL_PLANCK_C2*nu[i];
    }

    double rad[kPathWidth];
    if (l.starts)
    {
        const double tb = a.boundary_t[l.p - a.table_path];
        const double eb = a.boundary_e[l.p - a.table_path];
        if constexpr (kSurface)
        {
            const long long row = (long long)l.p*a.stride + l.j;
            double e[kPathWidth], d[kPathWidth];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                e[i] = eb;
                d[i] = 0.;
            }
            if (a.emissivity_rows != nullptr) path_load<kVector>(a.emissivity_rows + row, width, e);
            if (a.reflection != nullptr) path_load<kVector>(a.reflection + row, width, d);
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double b = planck(nu[i], c1nu3[i], c2nu[i], tb);
                const double emitted = e[i]*b;
                rad[i] = !(tb > 0.) ? 0. : a.reflection != nullptr ? emitted + (1. - e[i])*d[i]
                                                                   : emitted;
            }
        }
        else
        {
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                rad[i] = tb > 0. ? eb*planck(nu[i], c1nu3[i], c2nu[i], tb) : 0.;
            }
        }
    }
    else
    {
        path_load<kVector>(a.carry + (long long)l.p*a.stride + l.j, width, rad);
    }
    const bool per_level = a.level_rad != nullptr || a.level_bt != nullptr;
    // kLinear: B at the interface the lane's next level is entered through.
    const int side = entry_side(l.direction);
    const double * edge = kLinear ? a.edge + 2*(long long)l.index0 : nullptr;
    double b_in[kPathWidth];
    if (kLinear)
    {
        const double t = edge[side];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) b_in[i] = planck(nu[i], c1nu3[i], c2nu[i], t);
    }
    path_levels<kPathAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth], long long at)
                                                 {
        const double s = length[k*l.direction];
        if (kLinear)
        {
            const double t = edge[2*(long long)(k*l.direction) + (1 - side)];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double b_out = planck(nu[i], c1nu3[i], c2nu[i], t);
                rad[i] = linear_update(rad[i], s*b[i], b_in[i], b_out);
                b_in[i] = b_out;
            }
        }
        else
        {
            const double t = temperature[k*l.direction];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i)
            {
                const double x = s*b[i];
                rad[i] = rad[i]*exp(-x) + planck(nu[i], c1nu3[i], c2nu[i], t)*(-expm1(-x));
            }
        }
        if (per_level)
        {
            radiance_store<kVector>(a.level_rad, a.level_bt, at, width, rad, nu, c1nu3, c2nu);
        }
    });

    const long long row = (long long)l.p*a.stride + l.j;
    if (!l.finishes || a.keep_final) path_store<kVector>(a.carry + row, width, rad);
    if (l.finishes)
    {
        radiance_store<kVector>(a.final_rad, a.final_bt, row, width, rad, nu, c1nu3, c2nu);
    }
}

// grid and kVector as for path_sweep_kernel.  kLinear: the linear-in-tau source of a.edge.
template <bool kVector, bool kLinear = false>
__global__ __launch_bounds__(kPathThreads) void path_radiance_kernel(PathRadiance a)
{
    radiance_sweep<kVector, kLinear, false>(a);
}

// The kSurface instantiations: path_radiance_kernel with the start value of a surface that has
// a spectral emissivity and/or reflects (lbl_path_radiance_surface).
template <bool kVector, bool kLinear>
__global__ __launch_bounds__(kPathThreads) void path_radiance_surface_kernel(PathSurface a)
{
    radiance_sweep<kVector, kLinear, true>(a);
}

}  // namespace lbl
