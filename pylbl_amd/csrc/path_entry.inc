// lbl_path_compute: optical depth and transmittance along paths through a block of absorption
// coefficients in HBM (kernels: path.h).  Included by engine.hip after delivery.inc.
namespace {

// Where a run of flat levels [begin, end) leaves the paths it touches: the first path, how many,
// and whether the sweep's first path continues from its carry row (its first level in sweep
// order lies outside the run).
struct PathRun
{
    int first_path, paths;
    bool continues;
};

PathRun path_run(int begin, int end, int levels_per_path, bool from_last)
{
    PathRun r;
    r.first_path = begin/levels_per_path;
    r.paths = (end - 1)/levels_per_path - r.first_path + 1;
    r.continues = from_last ? end % levels_per_path != 0 : begin % levels_per_path != 0;
    return r;
}

bool aligned16(const void * p)
{
    return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// The bands of a call: band b is columns [band_start[b], band_start[b + 1]), cut at multiples of
// kPathSegment into segments.  Staged as 8-byte words after the call's other tables: band_start
// [n_bands + 1], each band's first segment [n_bands + 1], then the segments (begin, end).
struct PathBands
{
    int n_bands = 0;
    std::vector<long long> band_segment;
    long long n_segments = 0;

    // nullptr, or what is wrong with the bands.
    const char * check(int32_t bands, const int64_t * band_start, int64_t columns)
    {
        if (bands < 0 || (bands > 0 && band_start == nullptr))
        {
            return "n_bands < 0, or band_start is NULL.";
        }
        n_bands = bands;
        if (n_bands == 0) return nullptr;
        if (band_start[0] < 0 || band_start[n_bands] > columns)
        {
            return "band_start out of [0, columns].";
        }
        for (int b = 0; b < n_bands; ++b)
        {
            if (band_start[b + 1] < band_start[b]) return "band_start must not decrease.";
        }
        band_segment.resize((size_t)n_bands + 1);
        for (int b = 0; b < n_bands; ++b)
        {
            band_segment[b] = n_segments;
            for (long long c = band_start[b]; c < band_start[b + 1];
                 c = (c/kPathSegment + 1)*kPathSegment)
            {
                n_segments += 1;
            }
        }
        band_segment[n_bands] = n_segments;
        if (n_segments > std::numeric_limits<int32_t>::max()) return "too many segments.";
        return nullptr;
    }

    size_t words() const
    {
        return n_bands > 0 ? 2*((size_t)n_bands + 1) + 2*(size_t)n_segments : 0;
    }

    void stage(long long * table, const int64_t * band_start) const
    {
        if (n_bands == 0) return;
        long long * segments = table + 2*((size_t)n_bands + 1);
        long long s = 0;
        for (int b = 0; b <= n_bands; ++b)
        {
            table[b] = band_start[b];
            table[n_bands + 1 + b] = band_segment[b];
        }
        for (int b = 0; b < n_bands; ++b)
        {
            for (long long c = band_start[b]; c < band_start[b + 1];)
            {
                const long long next = std::min<long long>((c/kPathSegment + 1)*kPathSegment,
                                                           band_start[b + 1]);
                segments[2*s] = c;
                segments[2*s + 1] = next;
                s += 1;
                c = next;
            }
        }
    }

    // Queues out[r][b] = the mean over band b of row r of `values` (of exp(-value) with
    // `transmittance`) for `rows` rows `row_stride` apart.  d_table: the staged words on the device.
    void means(PathWorkspace & w, const long long * d_table, const double * values,
               long long row_stride, int rows, bool transmittance, double * out,
               hipStream_t stream) const
    {
        // Rows go in the grid's y dimension, at most kPathGridY per launch; the chunks run one
        // after the other on this stream and share the partial sums.
        const int chunk_rows = std::min(rows, kPathGridY);
        w.partial.reserve((size_t)chunk_rows*(size_t)std::max<long long>(n_segments, 1));
        const long long * d_band_start = d_table;
        const long long * d_band_segment = d_table + n_bands + 1;
        const PathSegment * d_segments =
            reinterpret_cast<const PathSegment *>(d_table + 2*((long long)n_bands + 1));
        for (int r0 = 0; r0 < rows; r0 += kPathGridY)
        {
            const int chunk = std::min(rows - r0, kPathGridY);
            if (n_segments > 0)
            {
                const dim3 partial_grid(
                    (unsigned)((n_segments + kPathWaves - 1)/kPathWaves), (unsigned)chunk);
                hipLaunchKernelGGL(path_band_partial_kernel, partial_grid,
                                   dim3(kPathThreads), 0, stream,
                                   values + (long long)r0*row_stride, row_stride,
                                   d_segments, (int)n_segments, transmittance ? 1 : 0,
                                   w.partial.data);
                HIP_TRY(hipGetLastError());
            }
            const dim3 mean_grid((unsigned)((n_bands + kPathThreads - 1)/kPathThreads),
                                 (unsigned)chunk);
            hipLaunchKernelGGL(path_band_mean_kernel, mean_grid, dim3(kPathThreads), 0,
                               stream, w.partial.data, (int)n_segments, d_band_segment,
                               d_band_start, (int)n_bands, out + (long long)r0*n_bands);
            HIP_TRY(hipGetLastError());
        }
    }
};

}  // namespace

extern "C" {

int lbl_path_compute(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                     int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                     int32_t level_count, const double * path_length, int32_t n_bands,
                     const int64_t * band_start, double * carry, double * optical_depth,
                     double * transmittance, int32_t flags)
{
    if (engine == nullptr) return LBL_BAD_ARGUMENT;
    EngineLock lock(engine->mutex);
    auto bad = [&](const char * what) {
        return fail(engine, LBL_BAD_ARGUMENT, std::string("lbl_path_compute: ") + what);
    };
    const bool want_tau = (flags & LBL_PATH_OPTICAL_DEPTH) != 0;
    const bool want_trans = (flags & LBL_PATH_TRANSMITTANCE) != 0;
    const bool cumulative = (flags & LBL_PATH_CUMULATIVE) != 0;
    const bool from_last = (flags & LBL_PATH_FROM_LAST) != 0;
    if (beta == nullptr || path_length == nullptr || carry == nullptr)
    {
        return bad("beta, path_length and carry must not be NULL.");
    }
    if (!want_tau && !want_trans) return bad("no quantity requested.");
    if ((want_tau && optical_depth == nullptr) || (want_trans && transmittance == nullptr))
    {
        return bad("an output requested by the flags is NULL.");
    }
    if (from_last && !cumulative) return bad("LBL_PATH_FROM_LAST needs LBL_PATH_CUMULATIVE.");
    if (columns < 1 || row_stride < columns) return bad("need 1 <= columns <= row_stride.");
    if (n_paths < 1 || levels_per_path < 1 ||
        (int64_t)n_paths*levels_per_path > (int64_t)std::numeric_limits<int32_t>::max())
    {
        return bad("need n_paths >= 1 and levels_per_path >= 1.");
    }
    const int levels = n_paths*levels_per_path;
    if (level_begin < 0 || level_count < 1 || level_count > levels - level_begin)
    {
        return bad("the run [level_begin, level_begin + level_count) is not inside the levels.");
    }
    const int level_end = level_begin + level_count;
    const PathRun run = path_run(level_begin, level_end, levels_per_path, from_last);
    if (run.continues != ((flags & LBL_PATH_CONTINUE) != 0))
    {
        return bad(run.continues ? "the run starts inside a path: LBL_PATH_CONTINUE is needed."
                                 : "the run starts a path: LBL_PATH_CONTINUE must not be set.");
    }
    for (int i = 0; i < level_count; ++i)
    {
        if (!(path_length[i] >= 0.) || !std::isfinite(path_length[i]))
        {
            return bad("path lengths must be finite and >= 0.");
        }
    }
    PathBands bands;
    if (const char * problem = bands.check(n_bands, band_start, columns)) return bad(problem);
    // Rows whose band means this call forms: every level of the run (cumulative) or the paths
    // the run finishes.
    int band_rows = 0, band_row0 = 0;
    if (n_bands > 0)
    {
        if (cumulative)
        {
            band_rows = level_count;
        }
        else
        {
            // (upward: path p finishes here when its last level, (p + 1) L - 1, is in the run)
            band_row0 = level_begin/levels_per_path;
            band_rows = std::max(level_end/levels_per_path - band_row0, 0);
        }
    }
    try
    {
        HIP_TRY(hipSetDevice(engine->device));
        PathWorkspace & w = engine->path;
        // The tables: lengths [level_count], then the bands' words.
        const size_t words = (size_t)level_count + bands.words();
        double * staged = w.stage(words);
        std::memcpy(staged, path_length, (size_t)level_count*8);
        bands.stage(reinterpret_cast<long long *>(staged + level_count), band_start);
        hipStream_t stream = engine->stream;
        // Ordered like a plain compute call: after everything queued on the other lanes (the
        // block's writers among them) -- by events when the caller does not wait, so that the
        // host keeps queueing.  A call kept back (LBL_DEFER_FINISH) may still have the block to
        // write: it is queued first.
        engine->finish_deferred();
        if (flags & LBL_ASYNC)
        {
            engine->join_lanes(stream);
        }
        else
        {
            for (int i = 1; i < kAllLanes; ++i) engine->lanes[i].drain();
        }
        w.upload(words, stream);
        const double * d_length = w.tables.data;
        const long long * d_table = reinterpret_cast<const long long *>(w.tables.data + level_count);

        PathSweep a;
        a.beta = beta;
        a.stride = row_stride;
        a.columns = columns;
        a.length = d_length;
        a.first = level_begin;
        a.count = level_count;
        a.row_base = level_begin;
        a.levels_per_path = levels_per_path;
        a.first_path = run.first_path;
        a.from_last = from_last ? 1 : 0;
        a.carry = carry;
        a.level_tau = a.level_trans = a.final_tau = a.final_trans = nullptr;
        a.keep_final = 0;
        if (cumulative && n_bands > 0)
        {
            a.level_tau = beta;         // in place: the band means read the rows back
        }
        else if (cumulative)
        {
            a.level_tau = want_tau ? optical_depth : nullptr;
            a.level_trans = want_trans ? transmittance : nullptr;
        }
        else if (n_bands > 0)
        {
            a.keep_final = 1;
        }
        else
        {
            a.final_tau = want_tau ? optical_depth : nullptr;
            a.final_trans = want_trans ? transmittance : nullptr;
        }
        const bool vector = row_stride % 2 == 0 && aligned16(beta) && aligned16(carry) &&
                            aligned16(a.level_tau) && aligned16(a.level_trans) &&
                            aligned16(a.final_tau) && aligned16(a.final_trans);
        const long long per_block = (long long)kPathThreads*kPathWidth;
        // Paths go in the grid's y dimension, at most kPathGridY of them per launch.
        for (int y0 = 0; y0 < run.paths; y0 += kPathGridY)
        {
            a.first_path = run.first_path + y0;
            const dim3 grid((unsigned)((columns + per_block - 1)/per_block),
                            (unsigned)std::min(run.paths - y0, kPathGridY));
            if (vector)
            {
                hipLaunchKernelGGL(path_sweep_kernel<true>, grid, dim3(kPathThreads), 0, stream, a);
            }
            else
            {
                hipLaunchKernelGGL(path_sweep_kernel<false>, grid, dim3(kPathThreads), 0, stream, a);
            }
            HIP_TRY(hipGetLastError());
        }
        const long long last_row = (long long)(level_count - 1)*row_stride + columns;
        // The block counts as written even where it is only read: the next call that writes it
        // (the lines of the next run, on another lane) must wait for this sweep.
        engine->lanes[0].note_write(beta, last_row*8, stream);
        if (a.level_tau != nullptr && a.level_tau != beta)
        {
            engine->lanes[0].note_write(a.level_tau, last_row*8, stream);
        }
        if (a.level_trans != nullptr) engine->lanes[0].note_write(a.level_trans, last_row*8, stream);
        engine->lanes[0].note_write(carry, ((long long)(n_paths - 1)*row_stride + columns)*8,
                                    stream);
        if (a.final_tau != nullptr)
        {
            engine->lanes[0].note_write(a.final_tau, ((long long)(n_paths - 1)*row_stride + columns)*8,
                                        stream);
        }
        if (a.final_trans != nullptr)
        {
            engine->lanes[0].note_write(a.final_trans, ((long long)(n_paths - 1)*row_stride + columns)*8,
                                        stream);
        }

        if (n_bands > 0 && band_rows > 0)
        {
            // Values: the run's rows of beta (cumulative, in place) or the finished paths' carry
            // rows; outputs [rows][n_bands] from the first row this call forms.
            const double * values = cumulative ? beta : carry + (long long)band_row0*row_stride;
            const long long out_row0 = cumulative ? 0 : band_row0;
            for (int q = 0; q < 2; ++q)
            {
                const bool trans = q == 1;
                if (!(trans ? want_trans : want_tau)) continue;
                double * out = (trans ? transmittance : optical_depth) + out_row0*n_bands;
                bands.means(w, d_table, values, (long long)row_stride, band_rows, trans, out,
                            stream);
                engine->lanes[0].note_write(out, (long long)band_rows*n_bands*8, stream);
            }
        }
        if (!(flags & LBL_ASYNC)) HIP_TRY(hipStreamSynchronize(stream));
    }
    catch (const HipFailure & f)
    {
        return fail(engine, LBL_ERROR, f.message);
    }
    return LBL_OK;
}

}  // extern "C"
