// Path optical depth and band means (Spectroscopy.compute_path, lbl_path_compute): what a user
// does with the "total" absorption block right after computing it, done where the block is.
//
//   tau_p(nu_j) = sum_l s_{p,l} beta_{p,l}(nu_j), added in the order of the sweep as
//   tau = tau + s*beta from tau = 0 (the TU builds with -ffp-contract=off: no FMA), so that the
//   result is bit for bit the numpy loop in the same order.
//
// path_sweep_kernel: one pass over the levels of a run.  A lane owns kPathWidth consecutive
// columns (one 16-byte load per row), keeps tau in registers, has kPathAhead rows in flight, and
// writes per-level (cumulative) and final results as they are formed.  The block is read once:
// the kernel is bound by HBM.
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

struct PathSweep
{
    const double * beta;        // row of flat level `row_base`; rows `stride` apart
    long long stride;           // row stride of beta, carry, level and final outputs [values]
    long long columns;
    const double * length;      // [count]: path length of flat level first + i
    int first, count;           // the flat levels of this launch
    int row_base;               // flat level of row 0 of beta and the level outputs
    int levels_per_path;
    int first_path;             // path of blockIdx.y == 0
    int from_last;              // sweep each path from its last level down
    double * carry;             // [paths][stride]: tau of a path between runs
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

// grid (columns / (kPathThreads*kPathWidth), paths touched by [first, first + count)).
// kVector: every row starts 16-byte aligned (even stride, aligned bases).
template <bool kVector>
__global__ __launch_bounds__(kPathThreads) void path_sweep_kernel(PathSweep a)
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

    double tau[kPathWidth];
    if (starts)
    {
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) tau[i] = 0.;
    }
    else
    {
        path_load<kVector>(a.carry + (long long)p*a.stride + j, width, tau);
    }
    const bool per_level = a.level_tau != nullptr || a.level_trans != nullptr;
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
#pragma unroll
            for (int i = 0; i < kPathWidth; ++i) tau[i] = tau[i] + s*b[u][i];
            if (per_level)
            {
                const long long at = level0 + (long long)(k + u)*row_step;
                if (a.level_tau != nullptr) path_store<kVector>(a.level_tau + at, width, tau);
                if (a.level_trans != nullptr) path_store_exp<kVector>(a.level_trans + at, width, tau);
            }
        }
    }
    for (; k < n; ++k)
    {
        double b[kPathWidth];
        path_load<kVector>(beta + (long long)k*row_step, width, b);
        const double s = length[k*direction];
#pragma unroll
        for (int i = 0; i < kPathWidth; ++i) tau[i] = tau[i] + s*b[i];
        if (per_level)
        {
            const long long at = level0 + (long long)k*row_step;
            if (a.level_tau != nullptr) path_store<kVector>(a.level_tau + at, width, tau);
            if (a.level_trans != nullptr) path_store_exp<kVector>(a.level_trans + at, width, tau);
        }
    }

    const long long row = (long long)p*a.stride + j;
    if (!finishes || a.keep_final) path_store<kVector>(a.carry + row, width, tau);
    if (finishes)
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
