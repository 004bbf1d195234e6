// lbl_path_solar_radiance: the sunlight a viewer above the atmosphere sees scattered towards it,
// one zenith cosine and one scattering angle per path, from the two-stream fluxes
// lbl_path_two_stream left in HBM (kernel: solar_radiance.h; band means: path.h).  Included by
// engine.hip after thermal_radiance_entry.inc; shares path_entry.inc's PathCall, TwoStreamCall,
// PathTables and PathBands.  lbl_path_solar_radiance_spectral
// (include/lbl_amd_scatterer_radiance.h): the same from the fluxes of
// lbl_path_two_stream_spectral on the grid `grid`, with twostream_entry.inc's ScattererTable.
namespace {

// Both entries.  name: the entry's; spectral: the scatterer's knot table on the grid `grid`, or
// null for the grey scatterer of the level table.
int path_solar_radiance(lbl_engine * engine, const char * name, double * beta, int64_t row_stride,
                        int64_t columns, int32_t n_paths, int32_t levels_per_path,
                        int32_t level_begin, int32_t level_count, const double * level_table,
                        int32_t grid, ScattererTable * spectral,
                        const double * solar_zenith_cosine, const double * view_cosine,
                        const double * scattering_cosine, const double * solar_row,
                        const double * rayleigh_row, const double * albedo_rows,
                        const double * albedo, const double * up_rows,
                        const double * direct_rows, const double * diffuse_rows, int32_t n_bands,
                        const int64_t * band_start, double * radiance_rows,
                        double * radiance_mean, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, name, row_stride, columns, n_paths, levels_per_path, level_begin,
                      level_count, flags};
        // One row per path.
        double * const rows[1] = {radiance_rows};
        double * const mean[1] = {radiance_mean};
        const TwoStreamCall two{call, 1, 0, rows, mean};
        if (beta == nullptr || level_table == nullptr || solar_zenith_cosine == nullptr ||
            view_cosine == nullptr || scattering_cosine == nullptr || solar_row == nullptr)
        {
            return call.bad("beta, level_table, solar_zenith_cosine, view_cosine, "
                            "scattering_cosine and solar_row must not be NULL.");
        }
        if ((albedo_rows == nullptr) == (albedo == nullptr))
        {
            return call.bad("the surface needs an albedo: albedo_rows or albedo, not both.");
        }
        if (up_rows == nullptr || direct_rows == nullptr || diffuse_rows == nullptr)
        {
            return call.bad("up_rows, direct_rows and diffuse_rows, the fluxes of "
                            "lbl_path_two_stream, must not be NULL.");
        }
        if (const char * problem = two.check_whole_paths()) return call.bad(problem);
        if (radiance_rows != nullptr)
        {
            for (const double * in : {(const double *)beta, up_rows, direct_rows, diffuse_rows,
                                      solar_row, rayleigh_row, albedo_rows})
            {
                if (radiance_rows == in)
                {
                    return call.bad("an output must be neither beta nor a flux row nor another "
                                    "input.");
                }
            }
        }
        if (radiance_mean != nullptr && radiance_rows == nullptr)
        {
            return call.bad("a band mean needs the rows it is the mean of.");
        }
        if (radiance_rows == nullptr) return call.bad("no output requested.");
        if (radiance_mean != nullptr && n_bands == 0) return call.bad("band means need n_bands > 0.");
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
            if (row[3] > 0. && !(row[4] < row[3]))
            {
                return call.bad("the level table needs h_c < w_c where w_c > 0.");
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
            if (!(view_cosine[p] > 0. && view_cosine[p] <= 1.))
            {
                return call.bad("view cosines must lie in (0, 1].");
            }
            if (!(scattering_cosine[p] >= -1. && scattering_cosine[p] <= 1.))
            {
                return call.bad("scattering cosines must lie in [-1, 1].");
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
        const size_t mu_at = tables.add(run.paths, view_cosine + run.first_path);
        const size_t cos_at = tables.add(run.paths, scattering_cosine + run.first_path);
        tables.add(bands, band_start);
        if (spectral != nullptr) spectral->stage(tables, level_count);
        const double * d_tables = call.begin(tables);

        const double * nu = spectral != nullptr ? call.grid->wavenumber.data : nullptr;
        const bool vector = path_vector(row_stride, {beta, solar_row, rayleigh_row, albedo_rows,
                                                     up_rows, direct_rows, diffuse_rows,
                                                     radiance_rows, nu});
        dispatch([&](auto knots) {
            constexpr bool kSpectral = decltype(knots)::value;
            SolarViewArguments<kSpectral> a;
            call.fill(a, beta, nullptr);
            a.level = d_tables + level_at;
            a.mu0 = d_tables + mu0_at;
            a.albedo = d_tables + albedo_at;
            a.table_path = run.first_path;
            a.solar = solar_row;
            a.sigma = rayleigh_row;
            a.albedo_rows = albedo_rows;
            a.work = nullptr;
            for (int q = 0; q < 4; ++q) a.level_out[q] = a.top_out[q] = nullptr;
            a.mu = d_tables + mu_at;
            a.cos_theta = d_tables + cos_at;
            a.up = up_rows;
            a.direct = direct_rows;
            a.diffuse = diffuse_rows;
            a.rad = radiance_rows;
            if constexpr (kSpectral)
            {
                a.scatterer = spectral->on_device(d_tables, nu);
                a.scatters = d_tables + spectral->scatters_at;
            }
            // Surface -> space: against the order space -> surface, which is from_last() (the
            // surface is level 0), as lbl_path_two_stream's up sweep.
            a.from_last = call.from_last() ? 0 : 1;
            two.sweep(a, vector, [](auto v) {
                return solar_view_kernel<decltype(v)::value, kSpectral>;
            });
        }, spectral != nullptr);
        // beta and the flux rows are only read; they count as written, like beta in every path
        // entry, so that the next call that writes them waits for this sweep.
        call.note_rows(beta, level_count);
        call.note_rows(up_rows, level_count);
        call.note_rows(direct_rows, level_count);
        call.note_rows(diffuse_rows, level_count);
        call.note_rows(radiance_rows, n_paths);
        call.means(bands, PathMeanRows::kStarted, radiance_rows, radiance_mean);
        return LBL_OK;
    });
}

}  // namespace

extern "C" {

int lbl_path_solar_radiance(lbl_engine * engine, double * beta, int64_t row_stride,
                            int64_t columns, int32_t n_paths, int32_t levels_per_path,
                            int32_t level_begin, int32_t level_count, const double * level_table,
                            const double * solar_zenith_cosine, const double * view_cosine,
                            const double * scattering_cosine, const double * solar_row,
                            const double * rayleigh_row, const double * albedo_rows,
                            const double * albedo, const double * up_rows,
                            const double * direct_rows, const double * diffuse_rows,
                            int32_t n_bands, const int64_t * band_start, double * radiance_rows,
                            double * radiance_mean, int32_t flags)
{
    return path_solar_radiance(
        engine, "lbl_path_solar_radiance", beta, row_stride, columns, n_paths, levels_per_path,
        level_begin, level_count, level_table, 0, nullptr, solar_zenith_cosine, view_cosine,
        scattering_cosine, solar_row, rayleigh_row, albedo_rows, albedo, up_rows, direct_rows,
        diffuse_rows, n_bands, band_start, radiance_rows, radiance_mean, flags);
}

int lbl_path_solar_radiance_spectral(
    lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns, int32_t n_paths,
    int32_t levels_per_path, int32_t level_begin, int32_t level_count, const double * level_table,
    int32_t grid, int32_t n_knots, const double * knot_wavenumber, const double * knot_optics,
    const double * solar_zenith_cosine, const double * view_cosine,
    const double * scattering_cosine, const double * solar_row, const double * rayleigh_row,
    const double * albedo_rows, const double * albedo, const double * up_rows,
    const double * direct_rows, const double * diffuse_rows, int32_t n_bands,
    const int64_t * band_start, double * radiance_rows, double * radiance_mean, int32_t flags)
{
    ScattererTable spectral{n_knots, knot_wavenumber, knot_optics};
    return path_solar_radiance(
        engine, "lbl_path_solar_radiance_spectral", beta, row_stride, columns, n_paths,
        levels_per_path, level_begin, level_count, level_table, grid, &spectral,
        solar_zenith_cosine, view_cosine, scattering_cosine, solar_row, rayleigh_row, albedo_rows,
        albedo, up_rows, direct_rows, diffuse_rows, n_bands, band_start, radiance_rows,
        radiance_mean, flags);
}

}  // extern "C"
