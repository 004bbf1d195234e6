// What the path entries share (lbl_path_compute here, lbl_path_radiance, lbl_path_jacobian,
// lbl_path_flux, lbl_path_solar) -- the checks of a run, of its bands, boundaries and knots, the
// staged tables, the PathLevels part of the kernel arguments, the launches, the choice of outputs
// and the band means --, what the three whole-path two-stream entries share beyond that
// (TwoStreamCall), and lbl_path_compute: optical depth and transmittance along paths through
// a block of absorption coefficients in HBM (kernels: path.h).  Included by engine.hip after
// slot_entry.inc (grid handles).
#include "dispatch.h"

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

// Rows [first, first + count): the paths whose first level p L (or, with `last`, whose last level
// (p + 1) L - 1) in storage order lies in [begin, end).
struct PathRows
{
    int first, count;
};

PathRows path_rows(int begin, int end, int levels_per_path, bool last)
{
    const int shift = last ? 0 : levels_per_path - 1;
    PathRows r;
    r.first = (begin + shift)/levels_per_path;
    r.count = std::max((end + shift)/levels_per_path - r.first, 0);
    return r;
}

// Whether all `count` values are finite and >= 0 (with `positive`: > 0).
bool finite_at_least_zero(const double * values, long long count, bool positive)
{
    for (long long i = 0; i < count; ++i)
    {
        const double v = values[i];
        if (!(positive ? v > 0. : v >= 0.) || !std::isfinite(v)) return false;
    }
    return true;
}

// nullptr, or what is wrong with the interface temperatures [level_count][2] (null: none) of a run
// that starts at flat level `level_begin` (lbl_path_radiance_source, lbl_path_flux_source): finite
// and > 0, and inside a path the far side of a level equal to the near side of the next -- the
// kernels carry B at a level's exit interface into the next level as its entry value.
const char * check_edge_temperatures(const double * edge, int level_begin, int level_count,
                                     int levels_per_path)
{
    if (edge == nullptr) return nullptr;
    if (!finite_at_least_zero(edge, 2*(long long)level_count, true))
    {
        return "edge temperatures must be finite and > 0.";
    }
    for (int r = 0; r + 1 < level_count; ++r)
    {
        const bool same_path = (level_begin + r + 1) % levels_per_path != 0;
        if (same_path && edge[2*r + 1] != edge[2*(r + 1)])
        {
            return "edge temperatures must be continuous within a path: [r][1] == [r + 1][0].";
        }
    }
    return nullptr;
}

// nullptr, or what is wrong with the boundary of path p (lbl_path_radiance_*, lbl_path_jacobian):
// its temperature (null: 0, no boundary) and its emissivity (null: 1).
const char * check_boundary(const double * temperature, const double * emissivity, int p)
{
    const double t = temperature != nullptr ? temperature[p] : 0.;
    const double e = emissivity != nullptr ? emissivity[p] : 1.;
    if (!(t >= 0.) || !std::isfinite(t))
    {
        return "boundary temperatures must be finite and >= 0 (0: no boundary).";
    }
    if (!(e >= 0. && e <= 1.)) return "boundary emissivities must lie in [0, 1].";
    return nullptr;
}

// nullptr, or what is wrong with the knots of a table (lbl_surface_emissivity, lbl_solar_spectrum).
const char * check_knots(const double * knot, int n_knots)
{
    for (int j = 0; j < n_knots; ++j)
    {
        if (!std::isfinite(knot[j]) || (j > 0 && !(knot[j] > knot[j - 1])))
        {
            return "knots must be finite and strictly ascending.";
        }
    }
    return nullptr;
}

// Every row starts 16-byte aligned: an even stride and aligned bases (null: not used).
bool path_vector(int64_t row_stride, std::initializer_list<const void *> bases)
{
    if (row_stride % 2 != 0) return false;
    for (const void * p : bases)
    {
        if ((reinterpret_cast<uintptr_t>(p) & 15) != 0) return false;
    }
    return true;
}

// The bands of a call: band b is columns [band_start[b], band_start[b + 1]), cut at multiples of
// kPathSegment into segments.  Staged as 8-byte words among the call's tables: band_start
// [n_bands + 1], each band's first segment [n_bands + 1], then the segments (begin, end).
struct PathBands
{
    int n_bands = 0;
    std::vector<long long> band_segment;
    long long n_segments = 0;
    size_t at = 0;              // where PathTables::add staged them among the call's words

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
    // `transmittance`) for `rows` rows `row_stride` apart, and records the write of `out`.
    // d_tables: the call's tables on the device.  sums: the sums in place of the means, added in
    // the same order (band_interval_sum_kernel, band_sort_pairs.h): 0 for a band without points.
    void means(lbl_engine * engine, const double * d_tables, const double * values,
               long long row_stride, int rows, bool transmittance, double * out,
               bool sums = false) const
    {
        if (rows <= 0) return;
        const long long * d_table = reinterpret_cast<const long long *>(d_tables + at);
        PathWorkspace & w = engine->path;
        hipStream_t stream = engine->stream;
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
            if (sums)
            {
                hipLaunchKernelGGL(band_interval_sum_kernel, mean_grid, dim3(kPathThreads), 0,
                                   stream, w.partial.data, (int)n_segments, d_band_segment,
                                   (int)n_bands, out + (long long)r0*n_bands);
            }
            else
            {
                hipLaunchKernelGGL(path_band_mean_kernel, mean_grid, dim3(kPathThreads), 0,
                                   stream, w.partial.data, (int)n_segments, d_band_segment,
                                   d_band_start, (int)n_bands, out + (long long)r0*n_bands);
            }
            HIP_TRY(hipGetLastError());
        }
        engine->lanes[0].note_write(out, (long long)rows*n_bands*8, stream);
    }
};

// The tables of a call, staged as 8-byte words in one block (one copy to the device per call).
struct PathTables
{
    std::vector<double> words;

    // Appends `count` words (copies of `values`, or zeros) and returns their offset.
    size_t add(size_t count, const void * values = nullptr)
    {
        const size_t at = words.size();
        words.resize(at + count);
        if (values != nullptr) std::memcpy(words.data() + at, values, count*8);
        return at;
    }

    void add(PathBands & bands, const int64_t * band_start)
    {
        bands.at = add(bands.words());
        bands.stage(reinterpret_cast<long long *>(words.data() + bands.at), band_start);
    }

    // Two values per path of the run: [run.paths] of `first`, then [run.paths] of `second`, each
    // its path's value or, where the pointer is null, the default.
    size_t add_pair(const PathRun & run, const double * first, double first_default,
                    const double * second, double second_default)
    {
        const size_t at = add(2*(size_t)run.paths);
        double * pair = words.data() + at;
        for (int i = 0; i < run.paths; ++i)
        {
            const int p = run.first_path + i;
            pair[i] = first != nullptr ? first[p] : first_default;
            pair[run.paths + i] = second != nullptr ? second[p] : second_default;
        }
        return at;
    }
};

// Where a sweep writes its two quantities (null: not wanted): after every level (cumulative) or
// where a path finishes, and with bands as fine rows for the means to read -- in place in beta
// (cumulative) or left in the carry rows (keep_final).
struct PathOutputs
{
    double * level[2] = {nullptr, nullptr};
    double * final[2] = {nullptr, nullptr};
    int keep_final = 0;

    PathOutputs(bool cumulative, bool banded, double * beta, double * first, double * second)
    {
        if (cumulative && banded)
        {
            level[0] = beta;            // in place: the band means read the rows back
        }
        else if (cumulative)
        {
            level[0] = first;
            level[1] = second;
        }
        else if (banded)
        {
            keep_final = 1;
        }
        else
        {
            final[0] = first;
            final[1] = second;
        }
    }
};

// The rows a band mean is taken of: every level of the run, or one row per path the run starts
// or finishes in sweep order.
enum class PathMeanRows { kLevels, kStarted, kFinished };

// One call of a path entry: its run, its checks and the steps every entry takes in order.
struct PathCall
{
    lbl_engine * engine;
    const char * name;          // the entry, the prefix of its messages
    int64_t row_stride, columns;
    int32_t n_paths, levels_per_path, level_begin, level_count, flags;
    const SpectralGrid * grid = nullptr;
    PathRun run = {};
    const double * d_tables = nullptr;      // begin()'s

    int bad(const char * what) const
    {
        return fail(engine, LBL_BAD_ARGUMENT, std::string(name) + ": " + what);
    }

    bool from_last() const { return (flags & LBL_PATH_FROM_LAST) != 0; }
    int level_end() const { return level_begin + level_count; }

    // nullptr, or what is wrong with the grid handle.
    const char * find_grid(int32_t handle)
    {
        grid = find_slot(engine->grids, handle);
        return grid == nullptr ? "unknown grid handle." : nullptr;
    }

    // nullptr, or what is wrong with the run, its LBL_PATH_CONTINUE flag or its lengths
    // [level_count][angles].  Fills `run`.
    const char * check(const double * length, int angles)
    {
        if (columns < 1 || row_stride < columns) return "need 1 <= columns <= row_stride.";
        if (grid != nullptr && grid->n < columns)
        {
            return "the grid has fewer than `columns` points.";
        }
        if (n_paths < 1 || levels_per_path < 1 ||
            (int64_t)n_paths*levels_per_path > (int64_t)std::numeric_limits<int32_t>::max() ||
            (int64_t)n_paths*angles > (int64_t)std::numeric_limits<int32_t>::max())
        {
            return "need n_paths >= 1 and levels_per_path >= 1.";
        }
        const int levels = n_paths*levels_per_path;
        if (level_begin < 0 || level_count < 1 || level_count > levels - level_begin)
        {
            return "the run [level_begin, level_begin + level_count) is not inside the levels.";
        }
        run = path_run(level_begin, level_end(), levels_per_path, from_last());
        if (run.continues != ((flags & LBL_PATH_CONTINUE) != 0))
        {
            return run.continues ? "the run starts inside a path: LBL_PATH_CONTINUE is needed."
                                 : "the run starts a path: LBL_PATH_CONTINUE must not be set.";
        }
        if (!finite_at_least_zero(length, (long long)level_count*angles, false))
        {
            return "path lengths must be finite and >= 0.";
        }
        return nullptr;
    }

    // Stages the tables and queues their copy to the device, ordered like a plain compute call:
    // after everything queued on the other lanes (the block's writers among them) -- by events
    // when the caller does not wait, so that the host keeps queueing.  A call kept back
    // (LBL_DEFER_FINISH) may still have the block to write: it is queued first.  Returns the
    // tables on the device.
    const double * begin(const PathTables & tables)
    {
        HIP_TRY(hipSetDevice(engine->device));
        PathWorkspace & w = engine->path;
        const size_t words = tables.words.size();
        std::memcpy(w.staged.refill(words), tables.words.data(), words*8);
        engine->finish_deferred();
        if (flags & LBL_ASYNC)
        {
            engine->join_lanes(engine->stream);
        }
        else
        {
            for (int i = 1; i < kAllLanes; ++i) engine->lanes[i].drain();
        }
        w.tables.reserve(words);
        w.staged.upload(w.tables.data, words, engine->stream);
        return d_tables = w.tables.data;
    }

    // What every sweep's arguments share: the run and its rows in `beta` and `carry`.
    void fill(PathLevels & a, const double * beta, double * carry) const
    {
        a.beta = beta;
        a.stride = row_stride;
        a.columns = columns;
        a.first = level_begin;
        a.count = level_count;
        a.row_base = level_begin;
        a.levels_per_path = levels_per_path;
        a.first_path = run.first_path;      // (every launch sets its own)
        a.from_last = from_last() ? 1 : 0;
        a.carry = carry;
    }

    // The same with a sweep's arguments: sets a.first_path and queues launch(grid).
    template <typename Launch>
    void launch(PathLevels & a, Launch launch_one) const
    {
        launch([&](const dim3 & grid, int first_path) {
            a.first_path = first_path;
            launch_one(grid);
        });
    }

    // Queues launch(grid, first path) for every kPathGridY paths of the run (the grid's y limit).
    template <typename Launch>
    void launch(Launch launch_one) const
    {
        const long long per_block = (long long)kPathThreads*kPathWidth;
        for (int y0 = 0; y0 < run.paths; y0 += kPathGridY)
        {
            const dim3 grid((unsigned)((columns + per_block - 1)/per_block),
                            (unsigned)std::min(run.paths - y0, kPathGridY));
            launch_one(grid, run.first_path + y0);
            HIP_TRY(hipGetLastError());
        }
    }

    // Records the write of `rows` rows of `p` (null: none) on the engine's stream.  The block
    // counts as written even where it is only read: the next call that writes it (the lines of
    // the next run, on another lane) must wait for the sweep.
    void note_rows(const double * p, long long rows) const
    {
        if (p == nullptr) return;
        engine->lanes[0].note_write(p, ((rows - 1)*row_stride + columns)*8, engine->stream);
    }

    // What a sweep with PathOutputs touches.
    void note_sweep(const double * beta, const double * carry, const PathOutputs & o) const
    {
        note_rows(beta, level_count);
        note_rows(o.level[0] != beta ? o.level[0] : nullptr, level_count);
        note_rows(o.level[1], level_count);
        note_rows(carry, n_paths);
        note_rows(o.final[0], n_paths);
        note_rows(o.final[1], n_paths);
    }

    // Queues the means over `bands` of the rows `which` of `values` into the same rows of `out`
    // (null, or no bands: nothing).  values: row 0 is flat level level_begin (kLevels) or path 0;
    // out likewise, n_bands per row.  In sweep order a run starts the paths whose first level it
    // holds and finishes those whose last level it holds; from_last() swaps the two.
    void means(const PathBands & bands, PathMeanRows which, const double * values, double * out,
               bool transmittance = false) const
    {
        if (out == nullptr || bands.n_bands == 0) return;
        PathRows rows{0, level_count};
        if (which != PathMeanRows::kLevels)
        {
            rows = path_rows(level_begin, level_end(), levels_per_path,
                             (which == PathMeanRows::kStarted) == from_last());
        }
        bands.means(engine, d_tables, values + (long long)rows.first*row_stride,
                    (long long)row_stride, rows.count, transmittance,
                    out + (long long)rows.first*bands.n_bands);
    }
};

// What the whole-path two-stream entries share (lbl_path_two_stream, lbl_path_thermal_two_stream,
// lbl_path_thermal_two_stream_source): `count` outputs, the first `per_level` of them rows below
// every level of the run and the rest rows at interface 0 of every path, each with its band mean
// (null: not wanted); an up sweep that leaves what lies below every level in the work rows, and a
// down sweep behind it that writes the outputs.  The checks return nullptr or what is wrong, in
// the order the entries call them.
struct TwoStreamCall
{
    PathCall & call;
    int count, per_level;
    double * const * rows;
    double * const * mean;

    const char * check_whole_paths() const
    {
        if (call.flags & ~(LBL_PATH_FROM_LAST | LBL_ASYNC))
        {
            return "only LBL_PATH_FROM_LAST and LBL_ASYNC may be set: a call takes whole paths.";
        }
        if (call.levels_per_path >= 1 && (call.level_begin % call.levels_per_path != 0 ||
                                          call.level_count % call.levels_per_path != 0))
        {
            return "the run must consist of whole paths: level_begin and level_count must be "
                   "multiples of levels_per_path.";
        }
        return nullptr;
    }

    const char * check_outputs(const double * beta, const double * work, int32_t n_bands) const
    {
        bool any = false;
        for (int q = 0; q < count; ++q)
        {
            any = any || rows[q] != nullptr;
            if (rows[q] != nullptr && (rows[q] == beta || rows[q] == work))
            {
                return "an output must be neither beta nor the work rows.";
            }
            if (mean[q] != nullptr && rows[q] == nullptr)
            {
                return "a band mean needs the rows it is the mean of.";
            }
            if (mean[q] != nullptr && n_bands == 0) return "band means need n_bands > 0.";
        }
        if (!any) return "no output requested.";
        if (work == beta) return "work must not be beta.";
        return nullptr;
    }

    // The level table [level_count][words]: its first column, the thicknesses, are the run's
    // lengths (call.check); the other columns follow.
    const char * check_levels(const double * level_table, int words) const
    {
        if (call.level_count < 1) return "need level_count >= 1.";
        std::vector<double> thickness((size_t)call.level_count);
        for (int r = 0; r < call.level_count; ++r)
        {
            thickness[(size_t)r] = level_table[(size_t)r*words];
        }
        if (const char * problem = call.check(thickness.data(), 1)) return problem;
        if (!finite_at_least_zero(level_table, (long long)call.level_count*words, false))
        {
            return "the level table must be finite and >= 0.";
        }
        return nullptr;
    }

    // Up from the surface, then down from space behind it on the same stream.  The order space ->
    // surface is from_last() (the surface is level 0); the up sweep runs against it.  up(v) and
    // down(v): the kernels for rows that are 16-byte aligned (v: std::true_type) or not.
    template <typename Args, typename Up, typename Down>
    void sweeps(Args & a, bool vector, Up up, Down down) const
    {
        const int down_order = call.from_last() ? 1 : 0;
        a.from_last = 1 - down_order;
        sweep(a, vector, up);
        a.from_last = down_order;
        sweep(a, vector, down);
    }

    template <typename Args, typename Kernel>
    void sweep(Args & a, bool vector, Kernel kernel) const
    {
        call.launch(a, [&](const dim3 & grid) {
            dispatch([&](auto v) {
                hipLaunchKernelGGL((kernel(v)), grid, dim3(kPathThreads), 0, call.engine->stream,
                                   a);
            }, vector);
        });
    }

    // Records what the sweeps touched and queues the means: every interface below a level of the
    // run; interface 0 of its (whole) paths.
    void finish(const PathBands & bands, const double * beta, const double * work) const
    {
        call.note_rows(beta, call.level_count);
        call.note_rows(work, 2*(long long)call.level_count);
        for (int q = 0; q < count; ++q)
        {
            call.note_rows(rows[q], q < per_level ? call.level_count : call.n_paths);
        }
        for (int q = 0; q < count; ++q)
        {
            call.means(bands, q < per_level ? PathMeanRows::kLevels : PathMeanRows::kStarted,
                       rows[q], mean[q]);
        }
    }
};

// The frame of a path entry: entry()'s and, without LBL_ASYNC, the wait for the call's work.
template <typename Body>
int path_entry(lbl_engine * engine, int32_t flags, Body body)
{
    return entry(engine, [&] {
        const int status = body();
        if (status != LBL_OK) return status;
        if (!(flags & LBL_ASYNC)) HIP_TRY(hipStreamSynchronize(engine->stream));
        return LBL_OK;
    });
}

}  // namespace

extern "C" {

int lbl_path_compute(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                     int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                     int32_t level_count, const double * path_length, int32_t n_bands,
                     const int64_t * band_start, double * carry, double * optical_depth,
                     double * transmittance, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_path_compute", row_stride, columns, n_paths, levels_per_path,
                      level_begin, level_count, flags};
        const bool want_tau = (flags & LBL_PATH_OPTICAL_DEPTH) != 0;
        const bool want_trans = (flags & LBL_PATH_TRANSMITTANCE) != 0;
        const bool cumulative = (flags & LBL_PATH_CUMULATIVE) != 0;
        if (beta == nullptr || path_length == nullptr || carry == nullptr)
        {
            return call.bad("beta, path_length and carry must not be NULL.");
        }
        if (!want_tau && !want_trans) return call.bad("no quantity requested.");
        if ((want_tau && optical_depth == nullptr) || (want_trans && transmittance == nullptr))
        {
            return call.bad("an output requested by the flags is NULL.");
        }
        if (call.from_last() && !cumulative)
        {
            return call.bad("LBL_PATH_FROM_LAST needs LBL_PATH_CUMULATIVE.");
        }
        if (const char * problem = call.check(path_length, 1)) return call.bad(problem);
        PathBands bands;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }

        PathTables tables;
        const size_t length_at = tables.add(level_count, path_length);
        tables.add(bands, band_start);
        const double * d_tables = call.begin(tables);

        PathSweep a;
        call.fill(a, beta, carry);
        a.length = d_tables + length_at;
        const PathOutputs o(cumulative, n_bands > 0, beta, want_tau ? optical_depth : nullptr,
                            want_trans ? transmittance : nullptr);
        a.level_tau = o.level[0];
        a.level_trans = o.level[1];
        a.final_tau = o.final[0];
        a.final_trans = o.final[1];
        a.keep_final = o.keep_final;
        const bool vector = path_vector(row_stride, {beta, carry, a.level_tau, a.level_trans,
                                                     a.final_tau, a.final_trans});
        call.launch(a, [&](const dim3 & grid) {
            dispatch([&](auto v) {
                hipLaunchKernelGGL(path_sweep_kernel<v.value>, grid, dim3(kPathThreads), 0,
                                   engine->stream, a);
            }, vector);
        });
        call.note_sweep(beta, carry, o);

        // Rows: every level of the run (cumulative, in place in beta) or the paths the run
        // finishes, from their carry rows.
        const PathMeanRows rows = cumulative ? PathMeanRows::kLevels : PathMeanRows::kFinished;
        const double * values = cumulative ? beta : carry;
        call.means(bands, rows, values, want_tau ? optical_depth : nullptr);
        call.means(bands, rows, values, want_trans ? transmittance : nullptr, true);
        return LBL_OK;
    });
}

}  // extern "C"
