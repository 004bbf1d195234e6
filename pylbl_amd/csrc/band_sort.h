// Band k-distributions (Spectroscopy.compute_kdistribution, lbl_band_distribution): every
// (row, band) segment of a block in HBM sorted ascending, in place, in the total order of the
// keys below.  The keys are integers, so the result is unique: any run cut, layout or repeated
// call gives the same bits.
//
//   key(u) = u ^ 0x8000000000000000 for a clear sign bit, ~u for a set one (u: the fp64 bits),
//   compared unsigned: -inf < negatives < -0 < +0 < positives < +inf < NaN with the sign clear.
//
// band_chunk_sort_kernel: one workgroup sorts one chunk of at most kSortChunk values of a segment
// in LDS, as keys, by a bitonic network.  A short chunk is padded with the maximal key up to the
// next power of two >= 8, and only that much of the network runs; only the real values are
// stored.  Every thread holds 8 keys whose indices differ in three consecutive bits [lo, lo + 3),
// lo a multiple of 3, and runs the (up to) three strides of those bits in registers between one
// LDS read and one LDS write of its keys: 28 LDS round trips for 4096 keys where a stride per
// round trip takes 78.  (Exchanging 8-byte keys between lanes costs two 4-byte DPP or permute
// moves per key and stride; a conflict-free ds_read_b64 / ds_write_b64 pair per three strides is
// cheaper and the same for every stride, so the network does not switch to wave_ops.h below 64.)
// Bank conflicts: key i lives in slot sort_slot(i), i with its bits 0..4 XORed with bits 5..7
// (b0^b5, b1^b6, b2^b7, b3^b6, b4^b7).  The 32 lanes of a half wavefront then read 32 different
// 8-byte slots modulo 32 (all 64 banks once) for lo = 0 (their indices differ in bits 3..7),
// lo = 3 (bits 0..2, 6, 7) and lo >= 6 and the coalesced loads and stores (bits 0..4).
// band_merge_kernel: pass p merges neighbouring sorted runs of kSortChunk*2^p values within a
// segment from one buffer to the other (merge path).  One workgroup writes one tile of
// kMergeTile outputs: two threads find the tile's two diagonal split points by binary search in
// HBM, the tile's inputs go to LDS as keys, every thread finds its own split in LDS and merges
// 8 outputs, which leave through LDS in coalesced stores.  A run without a partner -- and every
// segment that is already one run -- is copied through, so that every segment ends in the same
// buffer after the last pass.  The tiles of a segment are the same in every pass: the host
// stages one table per call, the same for all rows.  Nothing is atomic.
// band_quantile_kernel: one thread per (row, band, point) gathers two sorted values.
// The interval means are path.h's path_band_partial_kernel / path_band_mean_kernel.
// Every access is one 8-byte value per lane: rows of any stride and alignment.
#pragma once

#include <hip/hip_runtime.h>

namespace lbl {

constexpr int kSortThreads = 512;
constexpr int kSortPerThread = 8;                           // keys per thread and round trip
constexpr int kSortChunk = kSortThreads*kSortPerThread;     // 4096 keys: 32 KB of LDS
constexpr int kSortChunkBits = 12;
constexpr int kMergeThreads = 256;
constexpr int kMergePerThread = 8;
constexpr int kMergeTile = kMergeThreads*kMergePerThread;   // 2048 outputs: 16 KB of LDS
static_assert(kSortChunk == 1 << kSortChunkBits && kSortChunk % kMergeTile == 0, "tiles");

typedef unsigned long long SortKey;
constexpr SortKey kSortSign = 0x8000000000000000ull;
constexpr SortKey kSortMaxKey = ~0ull;

__host__ __device__ __forceinline__ SortKey sort_key(SortKey bits)
{
    return (bits & kSortSign) ? ~bits : bits ^ kSortSign;
}

__host__ __device__ __forceinline__ SortKey sort_bits(SortKey key)
{
    return (key & kSortSign) ? key ^ kSortSign : ~key;
}

__device__ __forceinline__ SortKey load_key(const double * p)
{
    return sort_key((SortKey)__double_as_longlong(*p));
}

__device__ __forceinline__ void store_key(double * p, SortKey key)
{
    *p = __longlong_as_double((long long)sort_bits(key));
}

// Where key i of a chunk or tile lives in LDS (see above): a permutation of every aligned 256.
__host__ __device__ __forceinline__ int sort_slot(int i)
{
    return i ^ ((i >> 5) & 7) ^ (((i >> 6) & 3) << 3);
}

// A chunk of a segment: `count` (1..kSortChunk) columns from `begin`.
struct SortChunk
{
    long long begin, count;
};

// A tile of a segment's outputs: the segment's first column, its length and the tile's offset
// (a multiple of kMergeTile) in it.
struct MergeTile
{
    long long begin, length, offset;
};

// One stride of the phase that sorts runs of 2^phase keys, on the 8 keys of a thread whose
// indices are base + (e << lo): keys e and e + D, D = 1, 2 or 4, are the stride 2^lo*D apart.
template <int D>
__device__ __forceinline__ void sort_stride(SortKey (&k)[kSortPerThread], int base, int lo,
                                            int phase)
{
#pragma unroll
    for (int e = 0; e < kSortPerThread; ++e)
    {
        if ((e & D) == 0)
        {
            const bool descending = (((base | (e << lo)) >> phase) & 1) != 0;
            const SortKey a = k[e], b = k[e | D];
            const bool swap = descending ? a < b : a > b;
            k[e] = swap ? b : a;
            k[e | D] = swap ? a : b;
        }
    }
}

// The strides 2^high ... 2^lo (lo <= high < lo + 3) of that phase.
__device__ __forceinline__ void sort_strides(SortKey (&k)[kSortPerThread], int base, int lo,
                                             int high, int phase)
{
    if (high - lo >= 2) sort_stride<4>(k, base, lo, phase);
    if (high - lo >= 1) sort_stride<2>(k, base, lo, phase);
    sort_stride<1>(k, base, lo, phase);
}

// grid (chunks, rows): sorts the chunk's values of row blockIdx.y of `source` into the same
// columns of `target` (which may be `source`).
__global__ __launch_bounds__(kSortThreads) void band_chunk_sort_kernel(
    const double * source, double * target, long long row_stride, const SortChunk * chunks)
{
    __shared__ SortKey keys[kSortChunk];
    const int t = (int)threadIdx.x;
    const SortChunk chunk = chunks[blockIdx.x];
    const int count = (int)chunk.count;
    const long long at = (long long)blockIdx.y*row_stride + chunk.begin;

    // The network's size: the next power of two >= count, 8 at least.
    int bits = 3;
    while ((1 << bits) < count) ++bits;
    const int size = 1 << bits;

    for (int i = t; i < size; i += kSortThreads)
    {
        keys[sort_slot(i)] = i < count ? load_key(source + at + i) : kSortMaxKey;
    }
    __syncthreads();

    SortKey k[kSortPerThread];
    // Phases 1..3 (runs of 2, 4 and 8 keys) in one round trip.
    {
        const int base = t << 3;
        if (base < size)
        {
#pragma unroll
            for (int e = 0; e < kSortPerThread; ++e) k[e] = keys[sort_slot(base | e)];
            for (int phase = 1; phase <= 3; ++phase) sort_strides(k, base, 0, phase - 1, phase);
#pragma unroll
            for (int e = 0; e < kSortPerThread; ++e) keys[sort_slot(base | e)] = k[e];
        }
        __syncthreads();
    }
    for (int phase = 4; phase <= bits; ++phase)
    {
        for (int lo = ((phase - 1)/3)*3; lo >= 0; lo -= 3)
        {
            // The thread's keys: t's bits below lo stay, the others move up past the three.
            const int base = ((t >> lo) << (lo + 3)) | (t & ((1 << lo) - 1));
            if (base < size)
            {
                const int high = min(lo + 2, phase - 1);
#pragma unroll
                for (int e = 0; e < kSortPerThread; ++e) k[e] = keys[sort_slot(base | (e << lo))];
                sort_strides(k, base, lo, high, phase);
#pragma unroll
                for (int e = 0; e < kSortPerThread; ++e) keys[sort_slot(base | (e << lo))] = k[e];
            }
            __syncthreads();
        }
    }

    double * out = target + at;
    for (int i = t; i < count; i += kSortThreads) store_key(out + i, keys[sort_slot(i)]);
}

// How many of the first `diagonal` outputs of merging a[0, na) and b[0, nb) come from a (ties
// take a first): merge path's split by binary search.
template <typename LoadA, typename LoadB>
__device__ __forceinline__ long long merge_split(LoadA load_a, long long na, LoadB load_b,
                                                 long long nb, long long diagonal)
{
    long long lo = diagonal > nb ? diagonal - nb : 0;
    long long hi = diagonal < na ? diagonal : na;
    while (lo < hi)
    {
        const long long mid = (lo + hi) >> 1;
        if (load_a(mid) <= load_b(diagonal - 1 - mid)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid (tiles, rows): the tile's outputs of the pass that merges runs of `run` values (a multiple
// of kMergeTile) of row blockIdx.y, from `source` to the same columns of `target`.
__global__ __launch_bounds__(kMergeThreads) void band_merge_kernel(
    const double * source, double * target, long long row_stride, const MergeTile * tiles,
    long long run)
{
    __shared__ SortKey keys[kMergeTile];
    __shared__ long long split[2];
    const int t = (int)threadIdx.x;
    const MergeTile tile = tiles[blockIdx.x];
    const long long row = (long long)blockIdx.y*row_stride + tile.begin;
    // The pair of runs the tile lies in: a = [pair, pair + na), b = [pair + na, pair + na + nb).
    const long long pair = tile.offset/(2*run)*(2*run);
    const long long left = tile.length - pair;
    const long long na = left < run ? left : run;
    const long long nb = left - na < run ? left - na : run;
    const long long d0 = tile.offset - pair;
    const int count = (int)(na + nb - d0 < kMergeTile ? na + nb - d0 : kMergeTile);
    const double * a = source + row + pair;
    const double * b = a + na;
    double * out = target + row + tile.offset;

    if (nb <= 0)
    {
        // A run without a partner: copied through.
        for (int i = t; i < count; i += kMergeThreads) out[i] = a[d0 + i];
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
        keys[sort_slot(i)] = i < ta ? load_key(a + a0 + i) : load_key(b + b0 + (i - ta));
    }
    __syncthreads();

    SortKey merged[kMergePerThread];
    const int first = t*kMergePerThread;
    if (first < count)
    {
        int ia = (int)merge_split([&](long long i) { return keys[sort_slot((int)i)]; }, ta,
                                  [&](long long i) { return keys[sort_slot(ta + (int)i)]; }, tb,
                                  first);
        int ib = first - ia;
        SortKey ka = ia < ta ? keys[sort_slot(ia)] : kSortMaxKey;
        SortKey kb = ib < tb ? keys[sort_slot(ta + ib)] : kSortMaxKey;
#pragma unroll
        for (int e = 0; e < kMergePerThread; ++e)
        {
            const bool from_a = ib >= tb || (ia < ta && ka <= kb);
            merged[e] = from_a ? ka : kb;
            if (from_a)
            {
                ia += 1;
                ka = ia < ta ? keys[sort_slot(ia)] : kSortMaxKey;
            }
            else
            {
                ib += 1;
                kb = ib < tb ? keys[sort_slot(ta + ib)] : kSortMaxKey;
            }
        }
    }
    __syncthreads();
    if (first < count)
    {
#pragma unroll
        for (int e = 0; e < kMergePerThread; ++e) keys[sort_slot(first + e)] = merged[e];
    }
    __syncthreads();
    for (int i = t; i < count; i += kMergeThreads) store_key(out + i, keys[sort_slot(i)]);
}

// grid (bands*points / kMergeThreads, rows): quantile[row][band][point] = k_i + f*(k_j - k_i) of
// the band's sorted values, i = index[band][point] (< 0: a band without points, NaN), j =
// min(i + 1, N - 1), f = fraction[band][point]; evaluated as written (the TU has no FMA).
__global__ __launch_bounds__(kMergeThreads) void band_quantile_kernel(
    const double * values, long long row_stride, const long long * band_start, int n_bands,
    int n_points, const long long * index, const double * fraction, double * quantile)
{
    const long long item = (long long)blockIdx.x*kMergeThreads + threadIdx.x;
    const long long items = (long long)n_bands*n_points;
    if (item >= items) return;
    const int band = (int)(item/n_points);
    const long long begin = band_start[band], n = band_start[band + 1] - begin;
    const long long i = index[item];
    double result = __builtin_nan("");
    if (i >= 0 && i < n)
    {
        const double * v = values + (long long)blockIdx.y*row_stride + begin;
        const long long j = i + 1 < n ? i + 1 : n - 1;
        const double ki = v[i], kj = v[j];
        result = ki + fraction[item]*(kj - ki);
    }
    quantile[(long long)blockIdx.y*items + item] = result;
}

}  // namespace lbl
