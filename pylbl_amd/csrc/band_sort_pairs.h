// Weighted band k-distributions (Spectroscopy.compute_kdistribution with weighting=,
// lbl_band_distribution_weighted): band_sort.h's segmented sort carrying a payload, the column
// offset j of every value inside its band, so that the permutation g -> nu survives the sort.
//
//   pi sorts the pairs (key(k_j), j) lexicographically, key() the integer key of band_sort.h:
//   numpy.argsort(keys, kind="stable").  No two pairs of a band are equal, so pi is unique: any
//   run cut, layout or repeated call gives the same bits, and the sorted values are those of
//   band_chunk_sort_kernel / band_merge_kernel bit for bit.
//
// band_pair_chunk_sort_kernel: band_chunk_sort_kernel's network -- the same chunks, the same
// three strides per LDS round trip -- on (key, u32 offset) pairs compared lexicographically.  The
// padding of a short chunk is the pair (kSortMaxKey, 0xFFFFFFFF): the NaN with the bits
// 0x7FFF...F has the key kSortMaxKey too, but no real offset reaches 2^32 - 1 (bands are held
// below 2^31 columns), so every pad sorts behind every real pair.
// LDS: the offsets are a second array, 4 bytes per pair, under the same slot map as the keys
// (offset i lives in offsets[sort_slot(i)]): 32 KB + 16 KB for a chunk.  The keys move exactly
// as in band_sort.h.  The offsets move by ds_read_b32 / ds_write_b32, which are served per half
// wavefront with bank = dword address mod 32: the 32 lanes of a half wavefront address 32
// different slots modulo 32 in every round trip (band_sort.h: lo = 0, lo = 3, lo >= 6 and the
// coalesced loads and stores), which for 4-byte slots is every one of the 32 banks once.  Pairs
// of 16 bytes would be read by ds_read_b128 in four groups of 16 lanes and need a slot map of
// their own for strides below 16; they would also take 64 KB for a chunk.
// band_pair_merge_kernel: band_merge_kernel's merge path on pairs, stable: where keys are
// equal the element of the lower run (a) goes first -- in the tile's two diagonal searches in
// HBM, in every thread's search in LDS and in the serial merge (a's key <= b's key takes a).
// Runs are contiguous column ranges of a band and each is in pair order already, so every offset
// of a is below every offset of b: "a first on equal keys" is the lexicographic order, and no
// offset is ever compared here.  Keys and offsets ping-pong together between two buffers each.
// band_weight_gather_kernel: one element per lane: W_i = w_pi(i) -- B(nu, T) of radiance.h at
// nu = grid[band start + pi(i)] and the row's T, or weight_row[band start + pi(i)] -- and
// WK_i = W_i*k_i, one rounding (the TU has no FMA).
// band_interval_sum_kernel: path_band_mean_kernel without its division: the segment partials of
// path_band_partial_kernel added in segment order; 0 for an interval without columns.
#pragma once

#include <hip/hip_runtime.h>

#include "band_sort.h"
#include "path.h"
#include "radiance.h"

namespace lbl {

typedef unsigned int SortOffset;
constexpr SortOffset kSortPadOffset = 0xFFFFFFFFu;
constexpr int kGatherPerTile = kMergeTile/kMergeThreads;    // gather blocks per merge tile

// A chunk of a band: `count` (1..kSortChunk) columns from `begin`, the first of them `first`
// columns behind the band's first.
struct PairChunk
{
    long long begin, count, first;
};

// Whether the pair (ka, oa) sorts behind (kb, ob).
__device__ __forceinline__ bool pair_behind(SortKey ka, SortOffset oa, SortKey kb, SortOffset ob)
{
    return ka > kb || (ka == kb && oa > ob);
}

// sort_stride of band_sort.h on pairs.
template <int D>
__device__ __forceinline__ void pair_stride(SortKey (&k)[kSortPerThread],
                                            SortOffset (&o)[kSortPerThread], int base, int lo,
                                            int phase)
{
#pragma unroll
    for (int e = 0; e < kSortPerThread; ++e)
    {
        if ((e & D) == 0)
        {
            const bool descending = (((base | (e << lo)) >> phase) & 1) != 0;
            const SortKey a = k[e], b = k[e | D];
            const SortOffset oa = o[e], ob = o[e | D];
            const bool swap = descending ? pair_behind(b, ob, a, oa) : pair_behind(a, oa, b, ob);
            k[e] = swap ? b : a;
            k[e | D] = swap ? a : b;
            o[e] = swap ? ob : oa;
            o[e | D] = swap ? oa : ob;
        }
    }
}

__device__ __forceinline__ void pair_strides(SortKey (&k)[kSortPerThread],
                                             SortOffset (&o)[kSortPerThread], int base, int lo,
                                             int high, int phase)
{
    if (high - lo >= 2) pair_stride<4>(k, o, base, lo, phase);
    if (high - lo >= 1) pair_stride<2>(k, o, base, lo, phase);
    pair_stride<1>(k, o, base, lo, phase);
}

// grid (chunks, rows): sorts the chunk's values of row blockIdx.y of `source` into the same
// columns of `target` (which may be `source`) and writes their offsets in the band to the same
// columns of row blockIdx.y of `index` (rows `index_stride` apart).
__global__ __launch_bounds__(kSortThreads) void band_pair_chunk_sort_kernel(
    const double * source, double * target, int * index, long long row_stride,
    long long index_stride, const PairChunk * chunks)
{
    __shared__ SortKey keys[kSortChunk];
    __shared__ SortOffset offsets[kSortChunk];
    const int t = (int)threadIdx.x;
    const PairChunk chunk = chunks[blockIdx.x];
    const int count = (int)chunk.count;
    const long long at = (long long)blockIdx.y*row_stride + chunk.begin;

    int bits = 3;
    while ((1 << bits) < count) ++bits;
    const int size = 1 << bits;

    for (int i = t; i < size; i += kSortThreads)
    {
        const int s = sort_slot(i);
        keys[s] = i < count ? load_key(source + at + i) : kSortMaxKey;
        offsets[s] = i < count ? (SortOffset)(chunk.first + i) : kSortPadOffset;
    }
    __syncthreads();

    SortKey k[kSortPerThread];
    SortOffset o[kSortPerThread];
    {
        const int base = t << 3;
        if (base < size)
        {
#pragma unroll
            for (int e = 0; e < kSortPerThread; ++e)
            {
                const int s = sort_slot(base | e);
                k[e] = keys[s];
                o[e] = offsets[s];
            }
            for (int phase = 1; phase <= 3; ++phase) pair_strides(k, o, base, 0, phase - 1, phase);
#pragma unroll
            for (int e = 0; e < kSortPerThread; ++e)
            {
                const int s = sort_slot(base | e);
                keys[s] = k[e];
                offsets[s] = o[e];
            }
        }
        __syncthreads();
    }
    for (int phase = 4; phase <= bits; ++phase)
    {
        for (int lo = ((phase - 1)/3)*3; lo >= 0; lo -= 3)
        {
            const int base = ((t >> lo) << (lo + 3)) | (t & ((1 << lo) - 1));
            if (base < size)
            {
                const int high = min(lo + 2, phase - 1);
#pragma unroll
                for (int e = 0; e < kSortPerThread; ++e)
                {
                    const int s = sort_slot(base | (e << lo));
                    k[e] = keys[s];
                    o[e] = offsets[s];
                }
                pair_strides(k, o, base, lo, high, phase);
#pragma unroll
                for (int e = 0; e < kSortPerThread; ++e)
                {
                    const int s = sort_slot(base | (e << lo));
                    keys[s] = k[e];
                    offsets[s] = o[e];
                }
            }
            __syncthreads();
        }
    }

    double * out = target + at;
    int * out_index = index + (long long)blockIdx.y*index_stride + chunk.begin;
    for (int i = t; i < count; i += kSortThreads)
    {
        const int s = sort_slot(i);
        store_key(out + i, keys[s]);
        out_index[i] = (int)offsets[s];
    }
}

// grid (tiles, rows): band_merge_kernel's pass on pairs: the tile's outputs of the pass that
// merges runs of `run` values of row blockIdx.y from `source` / `index_source` to the same
// columns of `target` / `index_target`.  Equal keys: a's first (merge_split and the merge below).
__global__ __launch_bounds__(kMergeThreads) void band_pair_merge_kernel(
    const double * source, double * target, const int * index_source, int * index_target,
    long long row_stride, long long index_stride, const MergeTile * tiles, long long run)
{
    __shared__ SortKey keys[kMergeTile];
    __shared__ SortOffset offsets[kMergeTile];
    __shared__ long long split[2];
    const int t = (int)threadIdx.x;
    const MergeTile tile = tiles[blockIdx.x];
    const long long row = (long long)blockIdx.y*row_stride + tile.begin;
    const long long index_row = (long long)blockIdx.y*index_stride + tile.begin;
    const long long pair = tile.offset/(2*run)*(2*run);
    const long long left = tile.length - pair;
    const long long na = left < run ? left : run;
    const long long nb = left - na < run ? left - na : run;
    const long long d0 = tile.offset - pair;
    const int count = (int)(na + nb - d0 < kMergeTile ? na + nb - d0 : kMergeTile);
    const double * a = source + row + pair;
    const double * b = a + na;
    const int * oa = index_source + index_row + pair;
    const int * ob = oa + na;
    double * out = target + row + tile.offset;
    int * out_index = index_target + index_row + tile.offset;

    if (nb <= 0)
    {
        // A run without a partner: copied through.
        for (int i = t; i < count; i += kMergeThreads)
        {
            out[i] = a[d0 + i];
            out_index[i] = oa[d0 + i];
        }
        return;
    }
    if (t == 0 || t == 64)
    {
        const long long diagonal = d0 + (t == 0 ? 0 : count);
        split[t == 0 ? 0 : 1] = merge_split([&](long long i) { return load_key(a + i); }, na,
                                            [&](long long i) { return load_key(b + i); }, nb,
                                            diagonal);
    }
    __syncthreads();
    const long long a0 = split[0], b0 = d0 - a0;
    const int ta = (int)(split[1] - a0), tb = count - ta;
    // The tile's inputs: a's at [0, ta), b's at [ta, count).
    for (int i = t; i < count; i += kMergeThreads)
    {
        const int s = sort_slot(i);
        keys[s] = i < ta ? load_key(a + a0 + i) : load_key(b + b0 + (i - ta));
        offsets[s] = (SortOffset)(i < ta ? oa[a0 + i] : ob[b0 + (i - ta)]);
    }
    __syncthreads();

    SortKey merged[kMergePerThread];
    SortOffset merged_offset[kMergePerThread];
    const int first = t*kMergePerThread;
    if (first < count)
    {
        int ia = (int)merge_split([&](long long i) { return keys[sort_slot((int)i)]; }, ta,
                                  [&](long long i) { return keys[sort_slot(ta + (int)i)]; }, tb,
                                  first);
        int ib = first - ia;
#pragma unroll
        for (int e = 0; e < kMergePerThread; ++e)
        {
            // (Past the tile's end, first + e >= count, both runs are used up: slot 0 is read
            // and the result never stored.)
            const int sa = sort_slot(ia < ta ? ia : 0);
            const int sb = sort_slot(ib < tb ? ta + ib : 0);
            const SortKey ka = keys[sa], kb = keys[sb];
            const bool from_a = ib >= tb || (ia < ta && ka <= kb);
            merged[e] = from_a ? ka : kb;
            merged_offset[e] = from_a ? offsets[sa] : offsets[sb];
            ia += from_a ? 1 : 0;
            ib += from_a ? 0 : 1;
        }
    }
    __syncthreads();
    if (first < count)
    {
#pragma unroll
        for (int e = 0; e < kMergePerThread; ++e)
        {
            if (first + e < count)
            {
                const int s = sort_slot(first + e);
                keys[s] = merged[e];
                offsets[s] = merged_offset[e];
            }
        }
    }
    __syncthreads();
    for (int i = t; i < count; i += kMergeThreads)
    {
        const int s = sort_slot(i);
        store_key(out + i, keys[s]);
        out_index[i] = (int)offsets[s];
    }
}

// grid (tiles*kGatherPerTile, rows), one element per lane: for column c = band start + i of row
// blockIdx.y, with j = index[c] (pi(i)) and k = values[c] (the sorted k_i),
//   weight[c] = weight_row[band start + j], or with weight_row null
//               B(grid[band start + j], temperature[blockIdx.y]);   weighted[c] = weight[c]*k.
// An offset outside the band (none leaves the sort) gives NaN and reads nothing.
__global__ __launch_bounds__(kMergeThreads) void band_weight_gather_kernel(
    const double * values, const int * index, long long row_stride, long long index_stride,
    const MergeTile * tiles, const double * grid, const double * temperature,
    const double * weight_row, double * weight, double * weighted)
{
    const MergeTile tile = tiles[blockIdx.x/kGatherPerTile];
    const long long i = tile.offset + (long long)(blockIdx.x % kGatherPerTile)*kMergeThreads +
                        threadIdx.x;
    if (i >= tile.length) return;
    const long long at = (long long)blockIdx.y*row_stride + tile.begin + i;
    const long long j = index[(long long)blockIdx.y*index_stride + tile.begin + i];
    double w = __builtin_nan("");
    if (j >= 0 && j < tile.length)
    {
        if (weight_row != nullptr)
        {
            w = weight_row[tile.begin + j];
        }
        else
        {
            const double nu = grid[tile.begin + j];
            w = planck(nu, ((LBL_PLANCK_C1*nu)*nu)*nu, LBL_PLANCK_C2*nu, temperature[blockIdx.y]);
        }
    }
    weight[at] = w;
    weighted[at] = w*values[at];
}

// grid (intervals / kPathThreads, rows): out[row][interval] = the interval's partials of
// path_band_partial_kernel added in segment order; 0 for an interval without columns.
__global__ __launch_bounds__(kPathThreads) void band_interval_sum_kernel(
    const double * partial, int n_segments, const long long * band_segment, int n_bands,
    double * out)
{
    const int band = (int)(blockIdx.x*kPathThreads + threadIdx.x);
    if (band >= n_bands) return;
    const double * row = partial + (long long)blockIdx.y*n_segments;
    double sum = 0.;
    for (long long s = band_segment[band]; s < band_segment[band + 1]; ++s) sum = sum + row[s];
    out[(long long)blockIdx.y*n_bands + band] = sum;
}

}  // namespace lbl
