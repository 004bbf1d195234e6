// Longwave fluxes (Spectroscopy.compute_flux, lbl_path_flux): the radiance of K angles swept
// through the "total" absorption block in HBM at once, down from space and back up from a
// Lambertian surface.
//
//   s_{l,k} = s_l/mu_k (host, fp64), x = s_{l,k}*beta_l
//   I_k = I_k*exp(-x) + B(nu, T_l)*(-expm1(-x))     (radiance.h's update, path length s_{l,k})
//   down: I_k = 0 at space; up: I_k = eps*B(nu, T_s) + (1 - eps)*R, R = sum_k w_k*I_k of the
//   down sweep at the surface; F = pi*(sum_k w_k*I_k), sums from k = 0 upward.
// kLinear (lbl_path_flux_source with edge temperatures): radiance.h's linear-in-tau update,
//   I_k = I_k*exp(-x) + (B_in*u_in + B_out*w), w = 1 - a/x in radiance.h's two-branch form,
//   with B_in and B_out shared by the K angles; each angle adds its division and its weight.
// The TU builds with -ffp-contract=off: every product and sum is rounded as written, and with
// K = 1 and w_0 = 1 the radiances are bit for bit path_radiance_kernel's.
//
// path_flux_kernel<kVector, K> runs on path.h's sweep skeleton with kFluxAhead<K> rows in flight:
// radiance.h's update for K radiances per column, a lane's K*kPathWidth radiances in registers;
// nu, C2*nu and C1*nu^3 are formed once, and B(nu, T_l) once per element and level for all K
// angles (the two divisions and the expm1 of Planck are what one angle of the radiance sweep
// spends most on).  s_{l,k}, T_l and w_k are the same for the whole wavefront.
// After each level the lane writes F to its level row; band means go through path.h's kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lbl_amd.h"
#include "path.h"
#include "radiance.h"

namespace lbl {

constexpr int kFluxMaxAngles = 8;
constexpr double kFluxPi = 3.141592653589793;       // numpy.pi

// Rows in flight: kPathAhead while the K radiances leave room for them (no scratch at any K:
// DESIGN.md section 15 lists the registers of every instantiation).
template <int K>
constexpr int kFluxAhead = K <= 4 ? kPathAhead : 4;

struct PathFlux : PathLevels
{
    const double * nu;          // [columns]: the grid [cm-1]
    const double * length;      // [count][K]: s_l/mu_k of flat level first + i [m]
    const double * weight;      // [K]: the angles' weights
    const double * temperature; // [count]: temperature of flat level first + i [K]
    const double * surface_t;   // [paths of the run]: surface temperature [K] (up sweep)
    const double * surface_e;   // [paths of the run]: surface emissivity (up sweep)
    int table_path;             // path of surface_t[0] / surface_e[0]
    int up;                     // up sweep: starts from the surface, not from space
    double * reflection;        // [paths][stride]: R (down sweep writes, up sweep reads), then
                                // the up sweep's flux at the surface interface
    double * level_flux;        // F after each level
    const double * edge;        // [count][2]: interface temperatures as PathRadiance's (kLinear),
                                // or null
};

// sum_k w_k*I_k from k = 0, for every column of the lane.
template <int K>
__device__ __forceinline__ void flux_sum(const double * weight, const double (&rad)[K][kPathWidth],
                                         double (&out)[kPathWidth])
{
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i) out[i] = weight[0]*rad[0][i];
#pragma unroll
    for (int k = 1; k < K; ++k)
    {
        const double w = weight[k];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) out[i] = out[i] + w*rad[k][i];
    }
}

// pi*(sum_k w_k*I_k) at offset `at` of `out`.
template <bool kVector, int K>
__device__ __forceinline__ void flux_store(double * out, long long at, int width,
                                           const double * weight,
                                           const double (&rad)[K][kPathWidth])
{
    double f[kPathWidth];
    flux_sum<K>(weight, rad, f);
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i) f[i] = kFluxPi*f[i];
    path_store<kVector>(out + at, width, f);
}

// One level of every angle: B(nu, T) once per column, then the K updates.
template <int K>
__device__ __forceinline__ void flux_level(const double * length, double t,
                                           const double (&b)[kPathWidth],
                                           const double (&nu)[kPathWidth],
                                           const double (&c1nu3)[kPathWidth],
                                           const double (&c2nu)[kPathWidth],
                                           double (&rad)[K][kPathWidth])
{
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        const double source = planck(nu[i], c1nu3[i], c2nu[i], t);
#pragma unroll
        for (int k = 0; k < K; ++k)
        {
            const double x = length[k]*b[i];
            rad[k][i] = rad[k][i]*exp(-x) + source*(-expm1(-x));
        }
    }
}

// One level of every angle with the linear-in-tau source: B at the exit interface once per
// column, which becomes b_in of the next level.
template <int K>
__device__ __forceinline__ void flux_level_linear(const double * length, double t_out,
                                                  const double (&b)[kPathWidth],
                                                  const double (&nu)[kPathWidth],
                                                  const double (&c1nu3)[kPathWidth],
                                                  const double (&c2nu)[kPathWidth],
                                                  double (&b_in)[kPathWidth],
                                                  double (&rad)[K][kPathWidth])
{
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        const double b_out = planck(nu[i], c1nu3[i], c2nu[i], t_out);
#pragma unroll
        for (int k = 0; k < K; ++k)
        {
            rad[k][i] = linear_update(rad[k][i], length[k]*b[i], b_in[i], b_out);
        }
        b_in[i] = b_out;
    }
}

// grid and kVector as for path_sweep_kernel.  kLinear: the linear-in-tau source of a.edge.
template <bool kVector, int K, bool kLinear = false>
__global__ __launch_bounds__(kPathThreads) void path_flux_kernel(PathFlux a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const double * length = a.length + (long long)l.index0*K;
    const double * temperature = a.temperature + l.index0;
    const int width = l.width;
    const long long row = (long long)l.p*a.stride + l.j;
    double * carry = a.carry + (long long)l.p*K*a.stride + l.j;

    double nu[kPathWidth], c1nu3[kPathWidth], c2nu[kPathWidth];
    path_load<kVector>(a.nu + l.j, width, nu);
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        c1nu3[i] = ((LBL_PLANCK_C1*nu[i])*nu[i])*nu[i];
        c2nu[i] = LBL_PLANCK_C2*nu[i];
    }

    double rad[K][kPathWidth];
    if (l.starts && a.up)
    {
        const double ts = a.surface_t[l.p - a.table_path];
        const double es = a.surface_e[l.p - a.table_path];
        double r[kPathWidth];
        path_load<kVector>(a.reflection + row, width, r);
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i)
        {
            const double start = es*planck(nu[i], c1nu3[i], c2nu[i], ts) + (1. - es)*r[i];
#pragma unroll
            for (int k = 0; k < K; ++k) rad[k][i] = start;
        }
        // The flux at the surface interface replaces R in the same lane's columns.
        flux_store<kVector, K>(a.reflection, row, width, a.weight, rad);
    }
    else if (l.starts)
    {
#pragma unroll
        for (int k = 0; k < K; ++k)
        {
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i) rad[k][i] = 0.;
        }
    }
    else
    {
#pragma unroll
        for (int k = 0; k < K; ++k) path_load<kVector>(carry + (long long)k*a.stride, width, rad[k]);
    }
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
    path_levels<kFluxAhead<K>, kVector>(a, l, [&](int k, const double (&b)[kPathWidth],
                                                  long long at) {
        if (kLinear)
        {
            flux_level_linear<K>(length + (long long)k*l.direction*K,
                                 edge[2*(long long)(k*l.direction) + (1 - side)], b, nu, c1nu3,
                                 c2nu, b_in, rad);
        }
        else
        {
            flux_level<K>(length + (long long)k*l.direction*K, temperature[k*l.direction], b, nu,
                          c1nu3, c2nu, rad);
        }
        flux_store<kVector, K>(a.level_flux, at, width, a.weight, rad);
    });

    if (!l.finishes)
    {
#pragma unroll
        for (int q = 0; q < K; ++q) path_store<kVector>(carry + (long long)q*a.stride, width, rad[q]);
    }
    else if (!a.up)
    {
        double r[kPathWidth];
        flux_sum<K>(a.weight, rad, r);
        path_store<kVector>(a.reflection + row, width, r);
    }
}

}  // namespace lbl
