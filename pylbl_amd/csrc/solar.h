// Sunlight without scattering (Spectroscopy.compute_solar, lbl_solar_spectrum, lbl_path_solar): the
// direct beam at every interface and the sunlight a Lambertian surface reflects to a viewer, in one
// sweep over the "total" absorption block in HBM.
//
//   S(nu) [W m-2 (cm-1)-1]: the solar irradiance at normal incidence, the distance factor included;
//   F0 = mu0*S;  tau = 0, tv = 0;  F at the interface that faces space = F0
//   for each level in order from space to the surface, a_l the solar slant length, v_l the view length:
//     tau = tau + a_l*beta_l;  tv = tv + v_l*beta_l;  F at the interface below the level = F0*exp(-tau)
//   reflected radiance = ((A*F0)/pi)*exp(-(tau + tv)),  pi = kFluxPi, tau and tv at the surface
// Both optical depths are added in the Sun's order, space to surface: one read of beta serves both
// beams.  The TU builds with -ffp-contract=off: every product and sum is rounded as written.
//
// path_solar_kernel<kVector, kView> runs on path.h's sweep skeleton with kPathAhead rows in flight:
// a lane keeps F0, tau and, with kView, tv of its kPathWidth columns in registers; a_l and v_l are
// the same for the whole wavefront.  Per element and level: one or two multiply-adds, one exp, one
// store to the interface row.  The lane that starts a path writes the space interface, the lane that
// finishes it the surface interface and the reflected radiance.  Between runs tau and tv live in
// the carry rows [paths][2][stride]; a launch always leaves them there.  The block is read once: the
// kernel is bound by HBM.
//
// solar_spectrum_kernel<kVector> fills the S row: scale*B(nu, T), scale*values on the grid, or scale
// times a table of knots interpolated as surface.h interpolates the emissivity (surface_interval and
// surface_value: the written formula exists once).  The table stays in HBM (up to 2^22 knots).  On
// an ascending grid a workgroup searches the knot interval of its first and of its last column once;
// where the knots between them fit LDS (kSurfaceMaxKnots) it stages that slice and every lane
// searches there.  Otherwise, and on a grid that is not ascending, every lane searches in HBM.
#pragma once

#include <hip/hip_runtime.h>

#include "flux.h"
#include "path.h"
#include "radiance.h"
#include "surface.h"

namespace lbl {

constexpr int kSolarMaxKnots = 1 << 22;

struct PathSolar : PathLevels
{
    const double * length;      // [count]: solar slant length of flat level first + i [m]
    const double * view;        // [count]: view length of flat level first + i [m] (kView)
    const double * mu0;         // [paths of the run]: cosine of the solar zenith angle
    const double * albedo;      // [paths of the run]: scalar albedo (kView without albedo_rows)
    int table_path;             // path of mu0[0] / albedo[0]
    const double * solar;       // [columns]: S on the grid
    const double * albedo_rows; // [paths][stride]: A per path and column, or null (kView)
    double * level_flux;        // F at the interface below each level, or null
    double * space;             // [paths][stride]: F at the space interface, or null
    double * surface;           // [paths][stride]: F at the surface interface, or null
    double * reflected;         // [paths][stride]: the reflected radiance (kView)
};

// F0*exp(-tau) at offset `at` of `out`.
template <bool kVector>
__device__ __forceinline__ void solar_store(double * out, long long at, int width,
                                            const double (&f0)[kPathWidth],
                                            const double (&tau)[kPathWidth])
{
    double f[kPathWidth];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i) f[i] = f0[i]*exp(-tau[i]);
    path_store<kVector>(out + at, width, f);
}

// grid and kVector as for path_sweep_kernel.  kView: the view lengths and the reflected radiance.
template <bool kVector, bool kView>
__global__ __launch_bounds__(kPathThreads) void path_solar_kernel(PathSolar a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const double * length = a.length + l.index0;
    const double * view = kView ? a.view + l.index0 : nullptr;
    const int width = l.width;
    const long long row = (long long)l.p*a.stride + l.j;
    double * carry = a.carry + 2*(long long)l.p*a.stride + l.j;

    double f0[kPathWidth];
    path_load<kVector>(a.solar + l.j, width, f0);
    const double mu0 = a.mu0[l.p - a.table_path];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i) f0[i] = mu0*f0[i];

    double tau[kPathWidth], tv[kPathWidth];
    if (l.starts)
    {
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) tau[i] = tv[i] = 0.;
        if (a.space != nullptr) path_store<kVector>(a.space + row, width, f0);
    }
    else
    {
        path_load<kVector>(carry, width, tau);
        if (kView) path_load<kVector>(carry + a.stride, width, tv);
    }
    path_levels<kPathAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth], long long at)
                                                 {
        const double s = length[k*l.direction];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) tau[i] = tau[i] + s*b[i];
        if (kView)
        {
            const double v = view[k*l.direction];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i) tv[i] = tv[i] + v*b[i];
        }
        if (a.level_flux != nullptr) solar_store<kVector>(a.level_flux, at, width, f0, tau);
    });

    path_store<kVector>(carry, width, tau);
    if (kView) path_store<kVector>(carry + a.stride, width, tv);
    if (!l.finishes) return;
    if (a.surface != nullptr) solar_store<kVector>(a.surface, row, width, f0, tau);
    if (kView)
    {
        double albedo[kPathWidth], r[kPathWidth];
        if (a.albedo_rows != nullptr)
        {
            path_load<kVector>(a.albedo_rows + row, width, albedo);
        }
        else
        {
            const double scalar = a.albedo[l.p - a.table_path];
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i) albedo[i] = scalar;
        }
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            r[i] = ((albedo[i]*f0[i])/kFluxPi)*exp(-(tau[i] + tv[i]));
        }
        path_store<kVector>(a.reflected + row, width, r);
    }
}

// What solar_spectrum_kernel fills the row from.
constexpr int kSolarBlackbody = 0;      // scale*B(nu, temperature)
constexpr int kSolarOnGrid = 1;         // scale*value[column]
constexpr int kSolarTable = 2;          // scale*(the table at nu)

struct SolarSpectrum
{
    const double * nu;          // [columns]: the grid [cm-1]
    long long columns;
    int mode;                   // kSolarBlackbody, kSolarOnGrid or kSolarTable
    const double * knot;        // kSolarTable: [n_knots] knots [cm-1], strictly ascending, in HBM
    const double * value;       // kSolarTable: [n_knots]; kSolarOnGrid: [columns]
    int n_knots;
    int ascending;              // the grid does not decrease: a workgroup may share its search
    double temperature, scale;
    double * row;               // [columns]
};

// The table at nu from the slice of `count` knots staged from knot `base` on: the interval of
// surface_interval among all m knots is found in the slice, which holds every knot from the last
// one <= the workgroup's first column to the first one > its last column.
__device__ __forceinline__ double solar_slice_value(const double * knot, const double * value,
                                                    int base, int count, int m,
                                                    const double * all_value, double nu)
{
    const int local = surface_interval(knot, count, nu);
    if (local < 0 && !(base > 0 && nu >= knot[0])) return all_value[0];    // nu <= k_0 (or NaN)
    const int at = local < 0 ? 0 : local;
    if (base + at >= m - 1) return value[count - 1];
    return surface_value(knot, value, count, at, nu);
}

// grid (columns / (kPathThreads*kPathWidth)).  kVector: the grid and the row are 16-byte aligned.
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void solar_spectrum_kernel(SolarSpectrum a)
{
    __shared__ double knot[kSurfaceMaxKnots];
    __shared__ double value[kSurfaceMaxKnots];
    const long long first = (long long)blockIdx.x*kPathThreads*kPathWidth;
    const long long j = first + (long long)threadIdx.x*kPathWidth;
    const bool active = j < a.columns;
    const int width = !active ? 0 :
        (int)(a.columns - j < kPathWidth ? a.columns - j : kPathWidth);
    double nu[kPathWidth] = {};
    if (active) path_load<kVector>(a.nu + j, width, nu);

    // kSolarTable on an ascending grid: the knots the workgroup's columns can fall between.
    const int m = a.n_knots;
    bool staged = false;
    int base = 0, count = 0;
    if (a.mode == kSolarTable && a.ascending)
    {
        const long long end = first + (long long)kPathThreads*kPathWidth < a.columns ?
            first + (long long)kPathThreads*kPathWidth : a.columns;
        const int lo = surface_interval(a.knot, m, a.nu[first]);
        const int hi = surface_interval(a.knot, m, a.nu[end - 1]);
        base = lo < 0 ? 0 : lo;
        const int last = hi + 1 < m - 1 ? hi + 1 : m - 1;
        count = last - base + 1;
        staged = count >= 1 && count <= kSurfaceMaxKnots;
        if (staged)
        {
            for (int i = (int)threadIdx.x; i < count; i += kPathThreads)
            {
                knot[i] = a.knot[base + i];
                value[i] = a.value[base + i];
            }
        }
        __syncthreads();        // (the condition is the same for the whole workgroup)
    }
    if (!active) return;

    double out[kPathWidth];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        double s;
        if (a.mode == kSolarBlackbody)
        {
            s = planck(nu[i], ((LBL_PLANCK_C1*nu[i])*nu[i])*nu[i], LBL_PLANCK_C2*nu[i],
                       a.temperature);
        }
        else if (a.mode == kSolarOnGrid)
        {
            s = i < width ? a.value[j + i] : 0.;
        }
        else if (staged)
        {
            s = solar_slice_value(knot, value, base, count, m, a.value, nu[i]);
        }
        else
        {
            s = surface_value(a.knot, a.value, m, surface_interval(a.knot, m, nu[i]), nu[i]);
        }
        out[i] = a.scale*s;
    }
    path_store<kVector>(a.row + j, width, out);
}

}  // namespace lbl
