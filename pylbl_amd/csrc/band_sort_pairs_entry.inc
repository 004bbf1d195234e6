// lbl_band_distribution_weighted (include/lbl_amd_kdist.h): lbl_band_distribution's sort carrying
// every value's column offset, the weights gathered through the permutation and their ordered
// interval sums (kernels: band_sort_pairs.h; the partial sums are path.h's).  On the frame of the
// path entries: included by engine.hip after band_sort_entry.inc.

namespace {

// BandSortPlan's with what the pairs add: every chunk's offset in its band, and the tiles staged
// for every call (the gather runs over them), whether a merge pass runs or not.
struct BandPairPlan
{
    std::vector<long long> chunks;      // (begin, count, first) per chunk
    std::vector<long long> tiles;       // (band begin, band length, offset) per tile
    int passes = 0;
    size_t chunks_at = 0, tiles_at = 0;

    long long n_chunks() const { return (long long)(chunks.size()/3); }
    long long n_tiles() const { return (long long)(tiles.size()/3); }

    // nullptr, or what is wrong.  band_start: checked (PathBands::check).
    const char * plan(const int64_t * band_start, int n_bands)
    {
        for (int b = 0; b < n_bands; ++b)
        {
            const long long begin = band_start[b], length = band_start[b + 1] - begin;
            if (length > std::numeric_limits<int32_t>::max())
            {
                return "a band is longer than 2^31 - 1 columns.";
            }
            for (long long c = 0; c < length; c += kSortChunk)
            {
                chunks.push_back(begin + c);
                chunks.push_back(std::min<long long>(length - c, kSortChunk));
                chunks.push_back(c);
            }
            for (long long o = 0; o < length; o += kMergeTile)
            {
                tiles.push_back(begin);
                tiles.push_back(length);
                tiles.push_back(o);
            }
            int needs = 0;
            while (((long long)kSortChunk << needs) < length) ++needs;
            passes = std::max(passes, needs);
        }
        if (n_chunks() > std::numeric_limits<int32_t>::max() ||
            n_tiles() > std::numeric_limits<int32_t>::max()/kGatherPerTile)
        {
            return "too many chunks.";
        }
        return nullptr;
    }
};

// Whether the blocks [p, p + p_bytes) and [q, q + q_bytes) share a byte (null: no).
bool blocks_overlap(const void * p, long long p_bytes, const void * q, long long q_bytes)
{
    if (p == nullptr || q == nullptr) return false;
    const char * a = static_cast<const char *>(p);
    const char * b = static_cast<const char *>(q);
    return a < b + q_bytes && b < a + p_bytes;
}

}  // namespace

extern "C" {

int lbl_band_distribution_weighted(
    lbl_engine * engine, double * values, int64_t row_stride, int64_t columns, int32_t n_rows,
    const int64_t * band_start, int32_t n_bands, double * scratch, int32_t grid,
    const double * row_temperature, const double * weight_row, int32_t * index_rows,
    int32_t * index_scratch, int64_t index_stride, double * weight_rows, double * weighted_rows,
    const int64_t * interval_start, int32_t n_intervals, double * weight_sums,
    double * weighted_sums, double * means, const int64_t * point_index,
    const double * point_fraction, int32_t n_points, double * quantiles, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_band_distribution_weighted", row_stride, columns, n_rows, 1, 0,
                      n_rows, flags};
        if (values == nullptr || index_rows == nullptr)
        {
            return call.bad("values and index_rows must not be NULL.");
        }
        if (n_bands < 1) return call.bad("need n_bands >= 1.");
        if (flags & ~LBL_ASYNC) return call.bad("flags: LBL_ASYNC or 0.");
        if ((row_temperature != nullptr) == (weight_row != nullptr))
        {
            return call.bad("exactly one of row_temperature and weight_row must be given.");
        }
        if (row_temperature != nullptr)
        {
            if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        }
        if (const char * problem = call.check(nullptr, 0)) return call.bad(problem);
        if (index_stride < columns) return call.bad("need index_stride >= columns.");
        if (row_temperature != nullptr && !finite_at_least_zero(row_temperature, n_rows, true))
        {
            return call.bad("row temperatures must be finite and > 0.");
        }
        PathBands bands, intervals;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }
        if ((weight_rows != nullptr) != (weighted_rows != nullptr))
        {
            return call.bad("weight_rows and weighted_rows go together.");
        }
        const bool want_sums = weight_sums != nullptr || weighted_sums != nullptr;
        if (want_sums && weight_rows == nullptr)
        {
            return call.bad("weight_sums and weighted_sums need weight_rows and weighted_rows.");
        }
        if ((want_sums || means != nullptr) != (n_intervals > 0))
        {
            return call.bad("means, weight_sums or weighted_sums and n_intervals > 0 go "
                            "together.");
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
        BandPairPlan plan;
        if (const char * problem = plan.plan(band_start, n_bands)) return call.bad(problem);
        if (plan.passes > 0 && (scratch == nullptr || index_scratch == nullptr))
        {
            return call.bad("a band is longer than 4096 columns: scratch and index_scratch must "
                            "not be NULL.");
        }
        // No two blocks of the call may share memory.
        const long long row_bytes = ((long long)(n_rows - 1)*row_stride + columns)*8;
        const long long index_bytes = ((long long)(n_rows - 1)*index_stride + columns)*4;
        const void * block[7] = {values, scratch, weight_rows, weighted_rows, weight_row,
                                 index_rows, index_scratch};
        const long long bytes[7] = {row_bytes, row_bytes, row_bytes, row_bytes, columns*8,
                                    index_bytes, index_bytes};
        for (int i = 0; i < 7; ++i)
        {
            for (int j = i + 1; j < 7; ++j)
            {
                if (blocks_overlap(block[i], bytes[i], block[j], bytes[j]))
                {
                    return call.bad("values, scratch, weight_rows, weighted_rows, weight_row, "
                                    "index_rows and index_scratch must not overlap.");
                }
            }
        }

        PathTables tables;
        tables.add(bands, band_start);
        tables.add(intervals, interval_start);
        plan.chunks_at = tables.add(plan.chunks.size(), plan.chunks.data());
        plan.tiles_at = tables.add(plan.tiles.size(), plan.tiles.data());
        const size_t points = want_quantiles ? (size_t)n_bands*(size_t)n_points : 0;
        const size_t index_at = tables.add(points, point_index);
        const size_t fraction_at = tables.add(points, point_fraction);
        const size_t temperature_at =
            tables.add(row_temperature != nullptr ? (size_t)n_rows : 0, row_temperature);
        const double * d_tables = call.begin(tables);
        hipStream_t stream = engine->stream;

        const PairChunk * d_chunks = reinterpret_cast<const PairChunk *>(d_tables + plan.chunks_at);
        const MergeTile * d_tiles = reinterpret_cast<const MergeTile *>(d_tables + plan.tiles_at);
        const long long * d_band_start = reinterpret_cast<const long long *>(d_tables + bands.at);
        const double * d_grid = row_temperature != nullptr ? call.grid->wavenumber.data : nullptr;
        // Rows go in the grid's y dimension, at most kPathGridY per launch.
        for (int r0 = 0; r0 < n_rows; r0 += kPathGridY)
        {
            const unsigned rows = (unsigned)std::min(n_rows - r0, kPathGridY);
            const long long at = (long long)r0*row_stride, index_row = (long long)r0*index_stride;
            double * here = values + at;
            double * there = scratch != nullptr ? scratch + at : nullptr;
            int * index_here = index_rows + index_row;
            int * index_there = index_scratch != nullptr ? index_scratch + index_row : nullptr;
            // After an even number of passes the results are back where the chunk sort put them:
            // keys and offsets take the same way.
            const bool even = plan.passes % 2 == 0;
            double * buffer[2] = {even ? here : there, even ? there : here};
            int * index_buffer[2] = {even ? index_here : index_there,
                                     even ? index_there : index_here};
            if (plan.n_chunks() > 0)
            {
                hipLaunchKernelGGL(band_pair_chunk_sort_kernel,
                                   dim3((unsigned)plan.n_chunks(), rows), dim3(kSortThreads), 0,
                                   stream, here, buffer[0], index_buffer[0],
                                   (long long)row_stride, (long long)index_stride, d_chunks);
                HIP_TRY(hipGetLastError());
            }
            for (int p = 0; p < plan.passes && plan.n_tiles() > 0; ++p)
            {
                hipLaunchKernelGGL(band_pair_merge_kernel, dim3((unsigned)plan.n_tiles(), rows),
                                   dim3(kMergeThreads), 0, stream, buffer[p % 2],
                                   buffer[(p + 1) % 2], index_buffer[p % 2],
                                   index_buffer[(p + 1) % 2], (long long)row_stride,
                                   (long long)index_stride, d_tiles, (long long)kSortChunk << p);
                HIP_TRY(hipGetLastError());
            }
            if (weight_rows != nullptr && plan.n_tiles() > 0)
            {
                hipLaunchKernelGGL(band_weight_gather_kernel,
                                   dim3((unsigned)(plan.n_tiles()*kGatherPerTile), rows),
                                   dim3(kMergeThreads), 0, stream, here, index_here,
                                   (long long)row_stride, (long long)index_stride, d_tiles, d_grid,
                                   row_temperature != nullptr ? d_tables + temperature_at + r0
                                                              : nullptr,
                                   weight_row, weight_rows + at, weighted_rows + at);
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
        call.note_rows(weight_rows, n_rows);
        call.note_rows(weighted_rows, n_rows);
        engine->lanes[0].note_write(index_rows, index_bytes, stream);
        if (plan.passes > 0)
        {
            call.note_rows(scratch, n_rows);
            engine->lanes[0].note_write(index_scratch, index_bytes, stream);
        }
        if (want_quantiles)
        {
            engine->lanes[0].note_write(quantiles, (long long)n_rows*(long long)points*8, stream);
        }
        if (means != nullptr)
        {
            intervals.means(engine, d_tables, values, (long long)row_stride, n_rows, false, means);
        }
        if (weight_sums != nullptr)
        {
            intervals.means(engine, d_tables, weight_rows, (long long)row_stride, n_rows, false,
                            weight_sums, true);
        }
        if (weighted_sums != nullptr)
        {
            intervals.means(engine, d_tables, weighted_rows, (long long)row_stride, n_rows, false,
                            weighted_sums, true);
        }
        return LBL_OK;
    });
}

}  // extern "C"
