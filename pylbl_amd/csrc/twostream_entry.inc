// lbl_rayleigh_row: the Rayleigh scattering cross-section on the grid, from the Bucholtz fit or
// from the caller's values; lbl_path_two_stream: two-stream shortwave fluxes at every interface of
// whole paths through a block of absorption coefficients in HBM (kernels: twostream.h; band
// means: path.h); lbl_path_two_stream_spectral: the same with the scatterer of every level as a
// table over wavenumber (include/lbl_amd_scatterer.h; kernels: scatterer.h).  Included by
// engine.hip after solar_entry.inc; shares path_entry.inc's PathCall, TwoStreamCall, PathTables
// and PathBands.  ScattererTable serves thermal_entry.inc too.
namespace {

// The knot table of a spectral scatterer as the two *_spectral entries take it: n_knots knots and
// [level_count][n_knots][3] optics (tau_c, omega_c, g_c) on the host.
struct ScattererTable
{
    int32_t n_knots;
    const double * knot;
    const double * optics;
    size_t knot_at = 0, optics_at = 0, scatters_at = 0;     // stage()'s, among the call's words

    // nullptr, or what is wrong with the table, or with the scatterer words [first_word,
    // first_word + 3) of the level table [level_count][words], which must be 0 beside it.
    const char * check(const double * level_table, int level_count, int words,
                       int first_word) const
    {
        if (n_knots < 2 || n_knots > kScattererMaxKnots)
        {
            return "n_knots must lie in 2 .. 1024.";
        }
        if (knot == nullptr || optics == nullptr)
        {
            return "knot_wavenumber and knot_optics must not be NULL.";
        }
        if (const char * problem = check_knots(knot, n_knots)) return problem;
        for (size_t i = 0; i < (size_t)level_count*(size_t)n_knots; ++i)
        {
            const double * e = optics + i*kScattererWords;
            if (!std::isfinite(e[0]) || !(e[0] >= 0.))
            {
                return "knot optical depths must be finite and >= 0.";
            }
            if (!(e[1] >= 0. && e[1] <= 1.))
            {
                return "knot single-scattering albedos must lie in [0, 1].";
            }
            if (!(e[2] >= 0. && e[2] < 1.)) return "knot asymmetries must lie in [0, 1).";
        }
        for (int r = 0; r < level_count; ++r)
        {
            for (int word = first_word; word < first_word + kScattererWords; ++word)
            {
                if (level_table[(size_t)r*words + word] != 0.)
                {
                    return "the scatterer words of the level table must be 0 beside a knot table.";
                }
            }
        }
        return nullptr;
    }

    // Whether level r scatters: some knot of it has omega_c*tau_c != 0.
    bool scatters(int r) const
    {
        const double * e = optics + (size_t)r*n_knots*kScattererWords;
        for (int j = 0; j < n_knots; ++j)
        {
            if (e[(size_t)j*kScattererWords + 1]*e[(size_t)j*kScattererWords] != 0.) return true;
        }
        return false;
    }

    // Appends the knots, the optics as the kernels read them, [level][3][n_knots], and one word
    // per level, 1 where it scatters and 0 where it is clear.
    void stage(PathTables & tables, int level_count)
    {
        knot_at = tables.add((size_t)n_knots, knot);
        const size_t m = (size_t)n_knots;
        optics_at = tables.add((size_t)level_count*kScattererWords*m);
        scatters_at = tables.add((size_t)level_count);
        for (int r = 0; r < level_count; ++r)
        {
            double * rows = tables.words.data() + optics_at + (size_t)r*kScattererWords*m;
            const double * level = optics + (size_t)r*m*kScattererWords;
            for (int word = 0; word < kScattererWords; ++word)
            {
                for (size_t j = 0; j < m; ++j) rows[word*m + j] = level[j*kScattererWords + word];
            }
            tables.words[scatters_at + (size_t)r] = scatters(r) ? 1. : 0.;
        }
    }

    ScattererKnots on_device(const double * d_tables, const double * nu) const
    {
        return ScattererKnots{nu, d_tables + knot_at, d_tables + optics_at, n_knots};
    }
};

// lbl_path_two_stream and, with a knot table (`spectral`, else null) on the grid `grid`,
// lbl_path_two_stream_spectral.  name: the entry's.
int path_two_stream(lbl_engine * engine, const char * name, double * beta, int64_t row_stride,
                    int64_t columns, int32_t n_paths, int32_t levels_per_path,
                    int32_t level_begin, int32_t level_count, const double * level_table,
                    int32_t grid, ScattererTable * spectral, const double * solar_zenith_cosine,
                    const double * solar_row, const double * rayleigh_row,
                    const double * albedo_rows, const double * albedo, int32_t n_bands,
                    const int64_t * band_start, double * work, double * const (&rows)[8],
                    double * const (&mean)[8], int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, name, row_stride, columns, n_paths, levels_per_path, level_begin,
                      level_count, flags};
        // Up, down, direct, diffuse: below each level, then at interface 0 of each path.
        constexpr int kRows = 8, kPerLevel = 4;
        const TwoStreamCall two{call, kRows, kPerLevel, rows, mean};
        if (beta == nullptr || level_table == nullptr || solar_zenith_cosine == nullptr ||
            solar_row == nullptr || work == nullptr)
        {
            return call.bad("beta, level_table, solar_zenith_cosine, solar_row and work must not "
                            "be NULL.");
        }
        if ((albedo_rows == nullptr) == (albedo == nullptr))
        {
            return call.bad("the surface needs an albedo: albedo_rows or albedo, not both.");
        }
        if (const char * problem = two.check_whole_paths()) return call.bad(problem);
        if (const char * problem = two.check_outputs(beta, work, n_bands))
        {
            return call.bad(problem);
        }
        if (spectral != nullptr)
        {
            if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        }
        if (const char * problem = two.check_levels(level_table, kTwoStreamLevelWords))
        {
            return call.bad(problem);
        }
        for (int r = 0; r < level_count; ++r)
        {
            const double * row = level_table + (size_t)r*kTwoStreamLevelWords;
            if (!(row[3] <= row[2]) || !(row[4] <= row[3]))
            {
                return call.bad("the level table needs h_c <= w_c <= tau_c.");
            }
        }
        for (int p = 0; p < n_paths; ++p)
        {
            const double mu0 = solar_zenith_cosine[p];
            if (!(mu0 > 0. && mu0 <= 1.)) return call.bad("solar zenith cosines must lie in (0, 1].");
            if (albedo != nullptr && !(albedo[p] >= 0. && albedo[p] <= 1.))
            {
                return call.bad("albedos must lie in [0, 1].");
            }
        }
        PathBands bands;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }
        if (spectral != nullptr)
        {
            if (const char * problem = spectral->check(level_table, level_count,
                                                       kTwoStreamLevelWords, 2))
            {
                return call.bad(problem);
            }
        }

        const PathRun & run = call.run;
        PathTables tables;
        const size_t level_at =
            tables.add((size_t)level_count*kTwoStreamLevelWords, level_table);
        const size_t mu0_at = tables.add(run.paths, solar_zenith_cosine + run.first_path);
        const size_t albedo_at =
            tables.add(run.paths, albedo != nullptr ? albedo + run.first_path : nullptr);
        tables.add(bands, band_start);
        if (spectral != nullptr) spectral->stage(tables, level_count);
        const double * d_tables = call.begin(tables);

        PathTwoStreamSpectral a;
        call.fill(a, beta, nullptr);
        a.level = d_tables + level_at;
        a.mu0 = d_tables + mu0_at;
        a.albedo = d_tables + albedo_at;
        a.table_path = run.first_path;
        a.solar = solar_row;
        a.sigma = rayleigh_row;
        a.albedo_rows = albedo_rows;
        a.work = work;
        for (int q = 0; q < kPerLevel; ++q)
        {
            a.level_out[q] = rows[q];
            a.top_out[q] = rows[kPerLevel + q];
        }
        const double * nu = spectral != nullptr ? call.grid->wavenumber.data : nullptr;
        const bool vector = path_vector(row_stride, {beta, solar_row, rayleigh_row, albedo_rows,
                                                     work, rows[0], rows[1], rows[2], rows[3],
                                                     rows[4], rows[5], rows[6], rows[7], nu});
        // The Sun's order is the down sweep's.
        if (spectral != nullptr)
        {
            a.scatterer = spectral->on_device(d_tables, nu);
            two.sweeps(a, vector, [](auto v) { return two_stream_up_kernel<v.value, true>; },
                       [](auto v) { return two_stream_down_kernel<v.value, true>; });
        }
        else
        {
            PathTwoStream & grey = a;
            two.sweeps(grey, vector, [](auto v) { return two_stream_up_kernel<v.value>; },
                       [](auto v) { return two_stream_down_kernel<v.value>; });
        }
        two.finish(bands, beta, work);
        return LBL_OK;
    });
}

}  // namespace

extern "C" {

int lbl_rayleigh_row(lbl_engine * engine, int32_t grid, int64_t columns,
                     const double * cross_section, double * row, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_rayleigh_row", columns, columns, 1, 1, 0, 1, flags};
        if (row == nullptr) return call.bad("row must not be NULL.");
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        if (columns < 1 || columns > call.grid->n)
        {
            return call.bad("need 1 <= columns <= the grid's points.");
        }
        if (cross_section != nullptr && !finite_at_least_zero(cross_section, columns, false))
        {
            return call.bad("cross-sections must be finite and >= 0.");
        }

        PathTables tables;
        const size_t value_at = tables.add(cross_section != nullptr ? columns : 0, cross_section);
        tables.add(1);                              // (never an empty copy)
        const double * d_tables = call.begin(tables);

        RayleighRow a;
        a.nu = call.grid->wavenumber.data;
        a.columns = columns;
        a.value = cross_section != nullptr ? d_tables + value_at : nullptr;
        a.row = row;
        const long long per_block = (long long)kPathThreads*kPathWidth;
        const dim3 launch((unsigned)((columns + per_block - 1)/per_block));
        dispatch([&](auto v) {
            hipLaunchKernelGGL(rayleigh_row_kernel<v.value>, launch, dim3(kPathThreads), 0,
                               engine->stream, a);
        }, path_vector(0, {row, a.nu, a.value}));
        HIP_TRY(hipGetLastError());
        call.note_rows(row, 1);
        return LBL_OK;
    });
}

int lbl_path_two_stream(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                        int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                        int32_t level_count, const double * level_table,
                        const double * solar_zenith_cosine, const double * solar_row,
                        const double * rayleigh_row, const double * albedo_rows,
                        const double * albedo, int32_t n_bands, const int64_t * band_start,
                        double * work, double * up_rows, double * down_rows,
                        double * direct_rows, double * diffuse_rows, double * top_up_rows,
                        double * top_down_rows, double * top_direct_rows,
                        double * top_diffuse_rows, double * up_mean, double * down_mean,
                        double * direct_mean, double * diffuse_mean, double * top_up_mean,
                        double * top_down_mean, double * top_direct_mean,
                        double * top_diffuse_mean, int32_t flags)
{
    return path_two_stream(
        engine, "lbl_path_two_stream", beta, row_stride, columns, n_paths, levels_per_path,
        level_begin, level_count, level_table, 0, nullptr, solar_zenith_cosine, solar_row,
        rayleigh_row, albedo_rows, albedo, n_bands, band_start, work,
        {up_rows, down_rows, direct_rows, diffuse_rows, top_up_rows, top_down_rows,
         top_direct_rows, top_diffuse_rows},
        {up_mean, down_mean, direct_mean, diffuse_mean, top_up_mean, top_down_mean,
         top_direct_mean, top_diffuse_mean}, flags);
}

int lbl_path_two_stream_spectral(
    lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns, int32_t n_paths,
    int32_t levels_per_path, int32_t level_begin, int32_t level_count, const double * level_table,
    int32_t grid, int32_t n_knots, const double * knot_wavenumber, const double * knot_optics,
    const double * solar_zenith_cosine, const double * solar_row, const double * rayleigh_row,
    const double * albedo_rows, const double * albedo, int32_t n_bands,
    const int64_t * band_start, double * work, double * up_rows, double * down_rows,
    double * direct_rows, double * diffuse_rows, double * top_up_rows, double * top_down_rows,
    double * top_direct_rows, double * top_diffuse_rows, double * up_mean, double * down_mean,
    double * direct_mean, double * diffuse_mean, double * top_up_mean, double * top_down_mean,
    double * top_direct_mean, double * top_diffuse_mean, int32_t flags)
{
    ScattererTable spectral{n_knots, knot_wavenumber, knot_optics};
    return path_two_stream(
        engine, "lbl_path_two_stream_spectral", beta, row_stride, columns, n_paths,
        levels_per_path, level_begin, level_count, level_table, grid, &spectral,
        solar_zenith_cosine, solar_row, rayleigh_row, albedo_rows, albedo, n_bands, band_start,
        work,
        {up_rows, down_rows, direct_rows, diffuse_rows, top_up_rows, top_down_rows,
         top_direct_rows, top_diffuse_rows},
        {up_mean, down_mean, direct_mean, diffuse_mean, top_up_mean, top_down_mean,
         top_direct_mean, top_diffuse_mean}, flags);
}

}  // extern "C"
