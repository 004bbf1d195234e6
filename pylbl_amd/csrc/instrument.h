// Instrument line shapes (Spectroscopy.compute_path / compute_radiance with `instrument`,
// lbl_instrument_apply): channel c of a row of fine-grid values v is
//
//   R_c = (sum_j w_c(nu_j - nu_c) v_j) / (sum_j w_c(nu_j - nu_c)),   start_c <= j < end_c,
//
// a weighted mean over the columns of the channel's window, normalised on the discrete grid.
// The weights do not depend on the row, and the windows of neighbouring channels overlap (about
// 12x for an IASI-like sounder).  So the host sorts the channels by window, cuts them into tiles
// of kInstrTile consecutive channels, and cuts the union of a tile's windows into segments of
// kInstrSegment columns (the segments that no window of the tile touches are dropped).  One
// workgroup takes one (tile, segment) item and a group of kInstrRowGroup rows:
//   - each wavefront owns kInstrTile/kInstrWaves channels of the tile; each lane forms the weights
//     of its columns of the segment for them once, in registers, and keeps them for every row of
//     the group;
//   - rows go through the LDS kInstrRows at a time: the workgroup reads the segment of those rows
//     once (exp(-v) formed there for transmittances), and every channel of the tile reads it from
//     the LDS instead of from HBM;
//   - each lane adds w*v over its columns in column order, wave_sums adds the 64 lanes in a fixed
//     pattern, and the item's partial sum of each (channel, row) goes to `partial`.
// instrument_mean_kernel then adds a channel's partials in segment order, and its weight sums
// (formed the same way by the workgroups of row group 0), and divides.  No atomics: repeated
// calls give the same bits, whatever the number of rows of a launch.
#pragma once

#include <hip/hip_runtime.h>

#include "wave_ops.h"

namespace lbl {

constexpr int kInstrThreads = 256;
constexpr int kInstrWaves = kInstrThreads/64;
constexpr int kInstrTile = 16;                          // channels per tile
constexpr int kInstrPerWave = kInstrTile/kInstrWaves;   // channels per wavefront
constexpr int kInstrSegment = 512;                      // columns per segment at most
constexpr int kInstrPerLane = kInstrSegment/64;         // columns per lane and segment
constexpr int kInstrRows = 8;                           // rows in the LDS at a time
constexpr int kInstrRowGroup = 64;                      // rows per workgroup

// Shapes of lbl_instrument_create (include/lbl_amd.h).
enum InstrShape : int
{
    kInstrBoxcar = 0,
    kInstrTriangle = 1,
    kInstrGaussian = 2,
    kInstrFts = 3,
    kInstrFtsHamming = 4,
    kInstrTabulated = 5,
};

// One channel, in the caller's order.  Staged as 8-byte words.
struct InstrChannel
{
    long long begin, end;       // window columns [begin, end)
    double center, parameter;   // nu_c; width, fwhm or max path difference L
    int valid;                  // 0: R_c is NaN (empty window, or not inside the grid)
    int row;                    // tabulated: its row of the response table
    int first_item, n_items;    // the items that hold its partials (consecutive)
    int slot;                   // its place in its tile, 0 .. kInstrTile - 1
    int pad;
};

// One (tile, segment) item: columns [begin, end) of the tile's channels.
struct InstrItem
{
    long long begin, end;
    long long tile;
};

struct InstrApply
{
    const double * values;      // row r at values + r*row_stride
    long long row_stride;
    int rows;                   // of this launch
    int transmittance;          // exp(-v) in place of v
    const double * nu;          // the grid the instrument was made for
    const InstrChannel * channel;
    const InstrItem * item;
    const long long * tile_channel;     // [tiles*kInstrTile]: channel of each slot, or -1
    int n_items, n_channels;
    int shape, n_table;
    const double * offsets;     // [n_table]
    const double * response;    // [rows of the table][n_table]
    double * partial;           // [rows][n_items*kInstrTile]
    double * weight_partial;    // [n_items*kInstrTile], written by row group 0
    double * out;               // [rows][n_channels]
};

__device__ __forceinline__ double instr_sinc(double x)
{
    if (x == 0.) return 1.;
    const double y = M_PI*x;
    return sin(y)/y;
}

// w(delta) of a channel: the formulas of Instrument.response (pylbl_amd/instrument.py), each
// product and sum rounded as written there.
__device__ __forceinline__ double instr_weight(const InstrApply & a, const InstrChannel & c,
                                               double d)
{
    const double p = c.parameter;
    switch (a.shape)
    {
    case kInstrBoxcar:
        return 1.;
    case kInstrTriangle:
        return 1. - fabs(d)/p;
    case kInstrGaussian:
    {
        const double x = d/p;
        return exp(-2.772588722239781*(x*x));          // 4 ln 2
    }
    case kInstrFts:
        return instr_sinc((2.*p)*d);
    case kInstrFtsHamming:
    {
        const double shift = 1./(2.*p);
        const double side = instr_sinc((2.*p)*(d - shift)) + instr_sinc((2.*p)*(d + shift));
        return 0.54*instr_sinc((2.*p)*d) + 0.23*side;
    }
    default:
    {
        // linear interpolation on the table, its end values outside it (numpy.interp)
        const double * o = a.offsets;
        const double * r = a.response + (long long)c.row*a.n_table;
        const int k = a.n_table;
        if (d <= o[0]) return r[0];
        if (d >= o[k - 1]) return r[k - 1];
        int lo = 0, hi = k - 1;                         // o[lo] < d < o[hi]
        while (hi - lo > 1)
        {
            const int mid = (lo + hi)/2;
            if (o[mid] <= d) lo = mid;
            else hi = mid;
        }
        if (o[lo] == d) return r[lo];
        const double slope = (r[lo + 1] - r[lo])/(o[lo + 1] - o[lo]);
        return slope*(d - o[lo]) + r[lo];
    }
    }
}

// grid (items, row groups of kInstrRowGroup).
__global__ __launch_bounds__(kInstrThreads) void instrument_partial_kernel(InstrApply a)
{
    __shared__ double stage[kInstrRows][kInstrSegment];
    const int lane = (int)threadIdx.x % 64;
    const int wave = (int)threadIdx.x/64;
    const InstrItem item = a.item[blockIdx.x];
    const long long width = item.end - item.begin;      // 1 .. kInstrSegment
    const long long slots = (long long)a.n_items*kInstrTile;

    // This lane's weights: channel k of the wave at column item.begin + lane + 64*m; `inside`
    // bit k*kInstrPerLane + m says whether that column is in the channel's window, bit k of
    // `active` whether channel k has columns in the item at all.
    double w[kInstrPerWave][kInstrPerLane];
    unsigned int inside = 0, active = 0;
    const long long * ids = a.tile_channel + item.tile*kInstrTile + wave*kInstrPerWave;
#pragma unroll
    for (int k = 0; k < kInstrPerWave; ++k)
    {
        if (ids[k] >= 0)
        {
            const InstrChannel & c = a.channel[ids[k]];
            if (c.begin < item.end && c.end > item.begin) active |= 1u << k;
        }
    }
    // Formed in a loop (one copy of the formulas) through the LDS, not yet holding rows: each
    // lane writes and reads back its own words, half of the wave's channels at a time.
    constexpr int kHalf = kInstrPerWave/2*kInstrPerLane;
    double * scratch = &stage[0][0] + (long long)wave*kHalf*64;
    static_assert(kInstrWaves*kHalf*64 <= kInstrRows*kInstrSegment, "scratch fits the stage");
#pragma unroll
    for (int half = 0; half < 2; ++half)
    {
#pragma unroll 1
        for (int f = 0; f < kHalf; ++f)
        {
            const int k = half*kInstrPerWave/2 + f/kInstrPerLane, m = f % kInstrPerLane;
            const long long j = item.begin + lane + 64*m;
            double weight = 0.;
            if ((active & (1u << k)) && j < item.end)
            {
                const InstrChannel c = a.channel[ids[k]];
                if (j >= c.begin && j < c.end)
                {
                    weight = instr_weight(a, c, a.nu[j] - c.center);
                    inside |= 1u << (k*kInstrPerLane + m);
                }
            }
            scratch[f*64 + lane] = weight;
        }
#pragma unroll
        for (int f = 0; f < kHalf; ++f)
        {
            w[half*kInstrPerWave/2 + f/kInstrPerLane][f % kInstrPerLane] = scratch[f*64 + lane];
        }
    }
    if (blockIdx.y == 0)
    {
        double sums[kInstrPerWave];
#pragma unroll
        for (int k = 0; k < kInstrPerWave; ++k)
        {
            double s = 0.;
#pragma unroll
            for (int m = 0; m < kInstrPerLane; ++m)
            {
                if (inside & (1u << (k*kInstrPerLane + m))) s = s + w[k][m];
            }
            sums[k] = s;
        }
        int index;
        bool valid;
        wave_sums(sums, index, valid);
        if (valid && (active & (1u << index)))
        {
            a.weight_partial[(long long)blockIdx.x*kInstrTile + wave*kInstrPerWave + index] =
                sums[0];
        }
    }

    const int row_begin = (int)blockIdx.y*kInstrRowGroup;
    const int row_end = min(row_begin + kInstrRowGroup, a.rows);
    for (int r0 = row_begin; r0 < row_end; r0 += kInstrRows)
    {
        const int here = min(kInstrRows, row_end - r0);
        __syncthreads();            // the previous rows have been read out of the LDS
        for (int e = (int)threadIdx.x; e < kInstrRows*kInstrSegment; e += kInstrThreads)
        {
            const int r = e/kInstrSegment, j = e % kInstrSegment;
            double v = 0.;
            if (r < here && j < width)
            {
                v = a.values[(long long)(r0 + r)*a.row_stride + item.begin + j];
                if (a.transmittance) v = exp(-v);
            }
            stage[r][j] = v;
        }
        __syncthreads();

        double sums[kInstrPerWave*kInstrRows];
#pragma unroll
        for (int i = 0; i < kInstrPerWave*kInstrRows; ++i) sums[i] = 0.;
#pragma unroll
        for (int m = 0; m < kInstrPerLane; ++m)
        {
            double v[kInstrRows];
#pragma unroll
            for (int r = 0; r < kInstrRows; ++r) v[r] = stage[r][lane + 64*m];
#pragma unroll
            for (int k = 0; k < kInstrPerWave; ++k)
            {
                if (inside & (1u << (k*kInstrPerLane + m)))
                {
#pragma unroll
                    for (int r = 0; r < kInstrRows; ++r)
                    {
                        sums[k*kInstrRows + r] = sums[k*kInstrRows + r] + w[k][m]*v[r];
                    }
                }
            }
        }
        int index;
        bool valid;
        wave_sums(sums, index, valid);
        const int k = index/kInstrRows, r = index % kInstrRows;
        if (valid && r < here && (active & (1u << k)))
        {
            a.partial[(long long)(r0 + r)*slots + (long long)blockIdx.x*kInstrTile +
                      wave*kInstrPerWave + k] = sums[0];
        }
    }
}

// grid (channels / kInstrThreads, rows): out[row][c] = the channel's partials added in segment
// order over its weights added in the same order; NaN for a channel that is not valid or whose
// weights do not sum to > 0.
__global__ __launch_bounds__(kInstrThreads) void instrument_mean_kernel(InstrApply a)
{
    const int id = (int)(blockIdx.x*kInstrThreads + threadIdx.x);
    if (id >= a.n_channels) return;
    const InstrChannel c = a.channel[id];
    double value = __builtin_nan("");
    if (c.valid)
    {
        const double * row = a.partial + (long long)blockIdx.y*a.n_items*kInstrTile;
        double sum = 0., weight = 0.;
        for (int i = c.first_item; i < c.first_item + c.n_items; ++i)
        {
            const long long at = (long long)i*kInstrTile + c.slot;
            sum = sum + row[at];
            weight = weight + a.weight_partial[at];
        }
        if (weight > 0.) value = sum/weight;
    }
    a.out[(long long)blockIdx.y*a.n_channels + id] = value;
}

}  // namespace lbl
