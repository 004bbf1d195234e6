// lbl_band_distribution: the (row, band) segments of a block in HBM sorted in place, their
// interval means and quantiles (kernels: band_sort.h; the means are path.h's).  On the frame of
// the path entries: included by engine.hip after path_entry.inc.

namespace {

// The sort of a call, the same for every row: the chunks of the first kernel, the tiles of the
// merge passes and how many passes the longest band needs.  Staged as 8-byte words.
struct BandSortPlan
{
    std::vector<long long> chunks;      // (begin, count) per chunk
    std::vector<long long> tiles;       // (band begin, band length, offset) per tile
    int passes = 0;
    size_t chunks_at = 0, tiles_at = 0;

    long long n_chunks() const { return (long long)(chunks.size()/2); }
    long long n_tiles() const { return (long long)(tiles.size()/3); }

    // nullptr, or what is wrong.  band_start: checked (PathBands::check).
    const char * plan(const int64_t * band_start, int n_bands)
    {
        for (int b = 0; b < n_bands; ++b)
        {
            const long long begin = band_start[b], length = band_start[b + 1] - begin;
            for (long long c = 0; c < length; c += kSortChunk)
            {
                chunks.push_back(begin + c);
                chunks.push_back(std::min<long long>(length - c, kSortChunk));
            }
            int needs = 0;
            while (((long long)kSortChunk << needs) < length) ++needs;
            passes = std::max(passes, needs);
        }
        if (passes > 0)
        {
            // Every band takes every pass: one that is a single run already is copied through.
            for (int b = 0; b < n_bands; ++b)
            {
                const long long begin = band_start[b], length = band_start[b + 1] - begin;
                for (long long o = 0; o < length; o += kMergeTile)
                {
                    tiles.push_back(begin);
                    tiles.push_back(length);
                    tiles.push_back(o);
                }
            }
        }
        if (n_chunks() > std::numeric_limits<int32_t>::max() ||
            n_tiles() > std::numeric_limits<int32_t>::max())
        {
            return "too many chunks.";
        }
        return nullptr;
    }
};

}  // namespace

extern "C" {

int lbl_band_distribution(lbl_engine * engine, double * values, int64_t row_stride,
                          int64_t columns, int32_t n_rows, const int64_t * band_start,
                          int32_t n_bands, double * scratch, const int64_t * interval_start,
                          int32_t n_intervals, double * means, const int64_t * point_index,
                          const double * point_fraction, int32_t n_points, double * quantiles,
                          int32_t flags)
{
    return path_entry(engine, flags, [&] {
        // One "path" of one level per row: PathCall's shape checks, ordering and write records.
        PathCall call{engine, "lbl_band_distribution", row_stride, columns, n_rows, 1, 0, n_rows,
                      flags};
        if (values == nullptr) return call.bad("values must not be NULL.");
        if (n_bands < 1) return call.bad("need n_bands >= 1.");
        if (flags & ~LBL_ASYNC) return call.bad("flags: LBL_ASYNC or 0.");
        if (const char * problem = call.check(nullptr, 0)) return call.bad(problem);
        PathBands bands, intervals;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }
        if ((means != nullptr) != (n_intervals > 0))
        {
            return call.bad("means and n_intervals > 0 go together.");
        }
        if (const char * problem = intervals.check(n_intervals, interval_start, columns))
        {
            return call.bad(problem);
        }
        const bool want_quantiles = quantiles != nullptr;
        if (n_points < 0 || want_quantiles != (n_points > 0) ||
            (want_quantiles && (point_index == nullptr || point_fraction == nullptr)))
        {
            return call.bad("quantiles, n_points > 0, point_index and point_fraction go "
                            "together.");
        }
        BandSortPlan plan;
        if (const char * problem = plan.plan(band_start, n_bands)) return call.bad(problem);
        if (plan.passes > 0 && scratch == nullptr)
        {
            return call.bad("a band is longer than 4096 columns: scratch must not be NULL.");
        }
        if (scratch == values) return call.bad("scratch must not be values.");

        PathTables tables;
        tables.add(bands, band_start);
        tables.add(intervals, interval_start);
        plan.chunks_at = tables.add(plan.chunks.size(), plan.chunks.data());
        plan.tiles_at = tables.add(plan.tiles.size(), plan.tiles.data());
        const size_t points = want_quantiles ? (size_t)n_bands*(size_t)n_points : 0;
        const size_t index_at = tables.add(points, point_index);
        const size_t fraction_at = tables.add(points, point_fraction);
        const double * d_tables = call.begin(tables);
        hipStream_t stream = engine->stream;

        const SortChunk * d_chunks = reinterpret_cast<const SortChunk *>(d_tables + plan.chunks_at);
        const MergeTile * d_tiles = reinterpret_cast<const MergeTile *>(d_tables + plan.tiles_at);
        const long long * d_band_start = reinterpret_cast<const long long *>(d_tables + bands.at);
        // Rows go in the grid's y dimension, at most kPathGridY per launch.
        for (int r0 = 0; r0 < n_rows; r0 += kPathGridY)
        {
            const unsigned rows = (unsigned)std::min(n_rows - r0, kPathGridY);
            double * here = values + (long long)r0*row_stride;
            double * there = scratch != nullptr ? scratch + (long long)r0*row_stride : nullptr;
            // After an even number of passes the result is back where the chunk sort put it.
            double * buffer[2] = {plan.passes % 2 == 0 ? here : there,
                                  plan.passes % 2 == 0 ? there : here};
            if (plan.n_chunks() > 0)
            {
                hipLaunchKernelGGL(band_chunk_sort_kernel, dim3((unsigned)plan.n_chunks(), rows),
                                   dim3(kSortThreads), 0, stream, here, buffer[0],
                                   (long long)row_stride, d_chunks);
                HIP_TRY(hipGetLastError());
            }
            for (int p = 0; p < plan.passes; ++p)
            {
                hipLaunchKernelGGL(band_merge_kernel, dim3((unsigned)plan.n_tiles(), rows),
                                   dim3(kMergeThreads), 0, stream, buffer[p % 2],
                                   buffer[(p + 1) % 2], (long long)row_stride, d_tiles,
                                   (long long)kSortChunk << p);
                HIP_TRY(hipGetLastError());
            }
            if (want_quantiles)
            {
                const unsigned blocks = (unsigned)((points + kMergeThreads - 1)/kMergeThreads);
                hipLaunchKernelGGL(band_quantile_kernel, dim3(blocks, rows), dim3(kMergeThreads),
                                   0, stream, here, (long long)row_stride, d_band_start,
                                   (int)n_bands, (int)n_points,
                                   reinterpret_cast<const long long *>(d_tables + index_at),
                                   d_tables + fraction_at, quantiles + (long long)r0*points);
                HIP_TRY(hipGetLastError());
            }
        }
        call.note_rows(values, n_rows);
        if (plan.passes > 0) call.note_rows(scratch, n_rows);
        if (want_quantiles)
        {
            engine->lanes[0].note_write(quantiles, (long long)n_rows*(long long)points*8, stream);
        }
        if (means != nullptr)
        {
            intervals.means(engine, d_tables, values, (long long)row_stride, n_rows, false, means);
        }
        return LBL_OK;
    });
}

}  // extern "C"
