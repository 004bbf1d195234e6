// Path optical depth and band means (Spectroscopy.compute_path, lbl_path_compute): what a user
// does with the "total" absorption block right after computing it, done where the block is.
//
//   tau_p(nu_j) = sum_l s_{p,l} beta_{p,l}(nu_j), added in the order of the sweep as
//   tau = tau + s*beta from tau = 0 (the TU builds with -ffp-contract=off: no FMA), so that the
//   result is bit for bit the numpy loop in the same order.
//
// The sweep skeleton, shared with path_radiance_kernel (radiance.h) and path_flux_kernel (flux.h):
// path_lane places a lane -- kPathWidth consecutive columns (one 16-byte load per row) of one path
// -- and path_levels runs its levels of the launch in sweep order with kAhead rows in flight,
// handing each row to the kernel's per-level update.  A kernel adds its state, its start, the
// update with its per-level stores, and its finish.
// path_sweep_kernel: tau in registers, per-level (cumulative) and final results written as they
// are formed.  The block is read once: the kernel is bound by HBM.
// path_band_partial_kernel / path_band_mean_kernel: arithmetic means over runs of columns.  The
// host cuts every band at multiples of kPathSegment columns; one wavefront sums one segment (each
// lane a fixed stride, then a fixed DPP scan), a second kernel adds a band's segment partials in
// segment order.  No atomics: repeated calls give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include "wave_ops.h"

namespace lbl {

constexpr int kPathThreads = 256;
constexpr int kPathWidth = 2;           // columns per lane: one double2 per row
constexpr int kPathAhead = 8;           // rows in flight per lane
constexpr int kPathSegment = 4096;      // columns per band segment at most (64 per lane)
constexpr int kPathWaves = kPathThreads/64;
constexpr int kPathGridY = 65535;       // paths or rows per launch (the grid's y limit)

// What the three sweeps (path_sweep_kernel, path_radiance_kernel in radiance.h,
// path_flux_kernel in flux.h) share of their arguments.
struct PathLevels
{
    const double * beta;        // row of flat level `row_base`; rows `stride` apart
    long long stride;           // row stride of beta, carry and the row outputs [values]
    long long columns;
    int first, count;           // the flat levels of this launch
    int row_base;               // flat level of row 0 of beta and the level outputs
    int levels_per_path;
    int first_path;             // path of blockIdx.y == 0
    int from_last;              // sweep each path from its last level down
    double * carry;             // [paths][stride] (flux: [paths][K][stride]): state between runs
};

struct PathSweep : PathLevels
{
    const double * length;      // [count]: path length of flat level first + i
    double * level_tau;         // cumulative: tau after each level (may be beta itself), or null
    double * level_trans;       // cumulative: exp(-tau) after each level, or null
    double * final_tau;         // [paths][stride]: tau of a finished path, or null
    double * final_trans;       // [paths][stride]: exp(-tau) of a finished path, or null
    int keep_final;             // a finished path's tau stays in its carry row (band means)
};

template <bool kVector>
__device__ __forceinline__ void path_load(const double * p, int width, double (&v)[kPathWidth])
{
    if (kVector && width == kPathWidth)
    {
        const double2 x = *reinterpret_cast<const double2 *>(p);
        v[0] = x.x;
        v[1] = x.y;
        return;
    }
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i) v[i] = i < width ? p[i] : 0.;
}

template <bool kVector>
__device__ __forceinline__ void path_store(double * p, int width, const double (&v)[kPathWidth])
{
    if (kVector && width == kPathWidth)
    {
        *reinterpret_cast<double2 *>(p) = make_double2(v[0], v[1]);
        return;
    }
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        if (i < width) p[i] = v[i];
    }
}

template <bool kVector>
__device__ __forceinline__ void path_store_exp(double * p, int width, const double (&tau)[kPathWidth])
{
    double t[kPathWidth];
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i) t[i] = exp(-tau[i]);
    path_store<kVector>(p, width, t);
}

// A lane's part of a sweep launch: columns [j, j + width) of path p, whose levels in the launch
// it takes in n steps -- step k is flat level lo + k upward, hi - 1 - k downward.
struct PathLane
{
    bool idle;                  // no columns, or no level of path p in the launch: nothing to do
    long long j;
    int width, p, n;
    bool starts, finishes;      // the path's first / last level in sweep order is in the launch
    int direction;              // +1 upward, -1 downward
    long long row_step;         // from one step's row to the next [values]
    long long level0;           // offset of step 0's row in beta and the level outputs
    int index0;                 // index of step 0 in the per-level tables (flat level - first)
};

// grid (columns / (kPathThreads*kPathWidth), paths touched by [first, first + count)).
__device__ __forceinline__ PathLane path_lane(const PathLevels & a)
{
    PathLane l;
    l.j = ((long long)blockIdx.x*kPathThreads + threadIdx.x)*kPathWidth;
    l.width = (int)(a.columns - l.j < kPathWidth ? a.columns - l.j : kPathWidth);
    l.p = a.first_path + (int)blockIdx.y;
    const int path_lo = l.p*a.levels_per_path, path_hi = path_lo + a.levels_per_path;
    const int lo = max(a.first, path_lo), hi = min(a.first + a.count, path_hi);
    l.idle = l.j >= a.columns || lo >= hi;
    l.starts = a.from_last ? hi == path_hi : lo == path_lo;
    l.finishes = a.from_last ? lo == path_lo : hi == path_hi;
    l.n = hi - lo;
    const int origin = a.from_last ? hi - 1 : lo;
    l.direction = a.from_last ? -1 : 1;
    l.row_step = (long long)l.direction*a.stride;
    l.level0 = (long long)(origin - a.row_base)*a.stride + l.j;
    l.index0 = origin - a.first;
    return l;
}

// The lane's levels in sweep order, kAhead rows in flight: step(k, b, at) with the step index,
// the lane's columns of its row of beta and the offset of that row in the level outputs.
template <int kAhead, bool kVector, typename Step>
__device__ __forceinline__ void path_levels(const PathLevels & a, const PathLane & l, Step step)
{
    const double * beta = a.beta + l.level0;
    int k = 0;
    for (; k + kAhead <= l.n; k += kAhead)
    {
        double b[kAhead][kPathWidth];
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
        {
            path_load<kVector>(beta + (long long)(k + u)*l.row_step, l.width, b[u]);
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
        {
            step(k + u, b[u], l.level0 + (long long)(k + u)*l.row_step);
        }
    }
    for (; k < l.n; ++k)
    {
        double b[kPathWidth];
        path_load<kVector>(beta + (long long)k*l.row_step, l.width, b);
        step(k, b, l.level0 + (long long)k*l.row_step);
    }
}

// kVector: every row starts 16-byte aligned (even stride, aligned bases).
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void path_sweep_kernel(PathSweep a)
{
    const PathLane l = path_lane(a);
    if (l.idle) return;
    const double * length = a.length + l.index0;
    const int width = l.width;

    double tau[kPathWidth];
    if (l.starts)
    {
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) tau[i] = 0.;
    }
    else
    {
        path_load<kVector>(a.carry + (long long)l.p*a.stride + l.j, width, tau);
    }
    const bool per_level = a.level_tau != nullptr || a.level_trans != nullptr;
    path_levels<kPathAhead, kVector>(a, l, [&](int k, const double (&b)[kPathWidth], long long at)
                                                 {
        const double s = length[k*l.direction];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) tau[i] = tau[i] + s*b[i];
        if (per_level)
        {
            if (a.level_tau != nullptr) path_store<kVector>(a.level_tau + at, width, tau);
            if (a.level_trans != nullptr) path_store_exp<kVector>(a.level_trans + at, width, tau);
        }
    });

    const long long row = (long long)l.p*a.stride + l.j;
    if (!l.finishes || a.keep_final) path_store<kVector>(a.carry + row, width, tau);
    if (l.finishes)
    {
        if (a.final_tau != nullptr) path_store<kVector>(a.final_tau + row, width, tau);
        if (a.final_trans != nullptr) path_store_exp<kVector>(a.final_trans + row, width, tau);
    }
}

// A run of columns [begin, end) of one band, at most kPathSegment long.
struct PathSegment
{
    long long begin, end;
};

// grid (segments / kPathWaves, rows): partial[row][segment] = sum over the segment of the row's
// values (or of exp(-value) with `transmittance`).
__global__ __launch_bounds__(kPathThreads) void path_band_partial_kernel(
    const double * values, long long row_step, const PathSegment * segments, int n_segments,
    int transmittance, double * partial)
{
    const int lane = (int)threadIdx.x % 64;
    const int segment = (int)blockIdx.x*kPathWaves + (int)threadIdx.x/64;
    if (segment >= n_segments) return;          // (whole wavefronts)
    const double * v = values + (long long)blockIdx.y*row_step;
    const PathSegment s = segments[segment];
    double sum = 0.;
    for (long long j = s.begin + lane; j < s.end; j += 64)
    {
        const double x = v[j];
        sum = sum + (transmittance ? exp(-x) : x);
    }
    sum = wave_prefix_sum(sum);
    if (lane == 63) partial[(long long)blockIdx.y*n_segments + segment] = sum;
}

// grid (bands / kPathThreads, rows): out[row][band] = the band's partials summed in segment
// order over its point count; NaN for a band without points.
__global__ __launch_bounds__(kPathThreads) void path_band_mean_kernel(
    const double * partial, int n_segments, const long long * band_segment,
    const long long * band_start, int n_bands, double * out)
{
    const int band = (int)(blockIdx.x*kPathThreads + threadIdx.x);
    if (band >= n_bands) return;
    const double * row = partial + (long long)blockIdx.y*n_segments;
    double sum = 0.;
    for (long long s = band_segment[band]; s < band_segment[band + 1]; ++s) sum = sum + row[s];
    const long long count = band_start[band + 1] - band_start[band];
    out[(long long)blockIdx.y*n_bands + band] = count > 0 ? sum/(double)count : __builtin_nan("");
}

}  // namespace lbl
