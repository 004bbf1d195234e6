// lbl_path_thermal_radiance: the radiance a viewer above the atmosphere sees through clouds, one
// zenith cosine per path, from the two-stream fluxes lbl_path_thermal_two_stream left in HBM
// (kernel: thermal_radiance.h; band means: path.h).  Included by engine.hip after
// thermal_entry.inc; shares path_entry.inc's PathCall, TwoStreamCall, PathTables and PathBands.
// lbl_path_thermal_radiance_spectral (include/lbl_amd_scatterer_radiance.h): the same from the
// fluxes of lbl_path_thermal_two_stream_spectral, with twostream_entry.inc's ScattererTable.
// lbl_path_thermal_radiance_source (include/lbl_amd_thermal_radiance_source.h): the same with the
// linear-in-tau source, from the fluxes of lbl_path_thermal_two_stream_source and its edge table
// (kernel: thermal_radiance_source.h; path_entry.inc's check_edge_temperatures).
namespace {

// All three entries.  name: the entry's; edge_temperature: [level_count][2] where `linear`, else
// null: the source of the level temperatures; spectral: the scatterer's knot table, or null for
// the grey scatterer of the level table (never with `linear`).
int path_thermal_radiance(lbl_engine * engine, const char * name, double * beta,
                          int64_t row_stride, int64_t columns, int32_t grid, int32_t n_paths,
                          int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                          const double * level_table, const double * edge_temperature,
                          bool linear, ScattererTable * spectral, double diffusivity,
                          const double * view_cosine,
                          const double * surface_temperature, const double * emissivity_rows,
                          const double * emissivity, const double * up_rows,
                          const double * down_rows, int32_t n_bands, const int64_t * band_start,
                          double * radiance_rows, double * brightness_rows,
                          double * radiance_mean, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, name, row_stride, columns, n_paths, levels_per_path, level_begin,
                      level_count, flags};
        // One row per path of each output; only the radiance has a band mean.
        double * const rows[2] = {radiance_rows, brightness_rows};
        double * const mean[2] = {radiance_mean, nullptr};
        const TwoStreamCall two{call, 2, 0, rows, mean};
        if (beta == nullptr || level_table == nullptr || (linear && edge_temperature == nullptr) ||
            view_cosine == nullptr || surface_temperature == nullptr)
        {
            return call.bad(linear ? "beta, level_table, edge_temperature, view_cosine and "
                                     "surface_temperature must not be NULL."
                                   : "beta, level_table, view_cosine and surface_temperature must "
                                     "not be NULL.");
        }
        if ((emissivity_rows == nullptr) == (emissivity == nullptr))
        {
            return call.bad("the surface needs an emissivity: emissivity_rows or emissivity, not "
                            "both.");
        }
        if (up_rows == nullptr || down_rows == nullptr)
        {
            return call.bad("up_rows and down_rows, the fluxes of lbl_path_thermal_two_stream, "
                            "must not be NULL.");
        }
        if (const char * problem = two.check_whole_paths()) return call.bad(problem);
        for (double * out : rows)
        {
            if (out != nullptr && (out == beta || out == up_rows || out == down_rows))
            {
                return call.bad("an output must be neither beta nor a flux row.");
            }
        }
        if (radiance_rows == nullptr && brightness_rows == nullptr)
        {
            return call.bad("no output requested.");
        }
        if (radiance_mean != nullptr && radiance_rows == nullptr)
        {
            return call.bad("a band mean needs the rows it is the mean of.");
        }
        if (radiance_mean != nullptr && n_bands == 0) return call.bad("band means need n_bands > 0.");
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        if (const char * problem = two.check_levels(level_table, kThermalLevelWords))
        {
            return call.bad(problem);
        }
        for (int r = 0; r < level_count; ++r)
        {
            const double * row = level_table + (size_t)r*kThermalLevelWords;
            if (!(row[2] <= row[1])) return call.bad("the level table needs w_c <= tau_c.");
            if (!(row[3] < 1.)) return call.bad("the level table needs g_c in [0, 1).");
            if (!(row[4] > 0.)) return call.bad("the level table needs T_l > 0.");
        }
        if (const char * problem = check_edge_temperatures(edge_temperature, level_begin,
                                                           level_count, levels_per_path))
        {
            return call.bad(problem);
        }
        if (!(diffusivity >= 1. && diffusivity <= 2.))
        {
            return call.bad("the diffusivity factor must lie in [1, 2].");
        }
        for (int p = 0; p < n_paths; ++p)
        {
            const double ts = surface_temperature[p];
            if (!(ts > 0.) || !std::isfinite(ts))
            {
                return call.bad("surface temperatures must be finite and > 0.");
            }
            if (emissivity != nullptr && !(emissivity[p] >= 0. && emissivity[p] <= 1.))
            {
                return call.bad("emissivities must lie in [0, 1].");
            }
            if (!(view_cosine[p] > 0. && view_cosine[p] <= 1.))
            {
                return call.bad("view cosines must lie in (0, 1].");
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
                                                       kThermalLevelWords, 1))
            {
                return call.bad(problem);
            }
        }

        const PathRun & run = call.run;
        PathTables tables;
        const size_t level_at = tables.add((size_t)level_count*kThermalLevelWords, level_table);
        const size_t ts_at = tables.add(run.paths, surface_temperature + run.first_path);
        const size_t eps_at =
            tables.add(run.paths, emissivity != nullptr ? emissivity + run.first_path : nullptr);
        const size_t mu_at = tables.add(run.paths, view_cosine + run.first_path);
        tables.add(bands, band_start);
        const size_t edge_at = tables.add(linear ? 2*(size_t)level_count : 0, edge_temperature);
        if (spectral != nullptr) spectral->stage(tables, level_count);
        const double * d_tables = call.begin(tables);

        const double * nu = call.grid->wavenumber.data;
        const bool vector = path_vector(row_stride, {beta, nu, emissivity_rows, up_rows,
                                                     down_rows, radiance_rows, brightness_rows});
        dispatch([&](auto knots) {
            constexpr bool kSpectral = decltype(knots)::value;
            ThermalViewArguments<kSpectral> a;
            call.fill(a, beta, nullptr);
            a.nu = nu;
            a.level = d_tables + level_at;
            a.diffusivity = diffusivity;
            a.surface_t = d_tables + ts_at;
            a.surface_e = d_tables + eps_at;
            a.table_path = run.first_path;
            a.emissivity_rows = emissivity_rows;
            a.work = nullptr;
            a.edge = linear ? d_tables + edge_at : nullptr;
            for (int q = 0; q < 2; ++q) a.level_out[q] = a.top_out[q] = nullptr;
            a.mu = d_tables + mu_at;
            a.up = up_rows;
            a.down = down_rows;
            a.rad = radiance_rows;
            a.bt = brightness_rows;
            if constexpr (kSpectral)
            {
                a.scatterer = spectral->on_device(d_tables, nu);
                a.scatters = d_tables + spectral->scatters_at;
            }
            // Surface -> space: against the order space -> surface, which is from_last() (the
            // surface is level 0), as lbl_path_thermal_two_stream's up sweep.
            a.from_last = call.from_last() ? 0 : 1;
            if constexpr (!kSpectral)
            {
                if (linear)
                {
                    two.sweep(a, vector, [](auto v) {
                        return thermal_view_source_kernel<decltype(v)::value>;
                    });
                    return;
                }
            }
            two.sweep(a, vector, [](auto v) {
                return thermal_view_kernel<decltype(v)::value, kSpectral>;
            });
        }, spectral != nullptr);
        // beta and the flux rows are only read; they count as written, like beta in every path
        // entry, so that the next call that writes them waits for this sweep.
        call.note_rows(beta, level_count);
        call.note_rows(up_rows, level_count);
        call.note_rows(down_rows, level_count);
        call.note_rows(radiance_rows, n_paths);
        call.note_rows(brightness_rows, n_paths);
        call.means(bands, PathMeanRows::kStarted, radiance_rows, radiance_mean);
        return LBL_OK;
    });
}

}  // namespace

extern "C" {

int lbl_path_thermal_radiance(lbl_engine * engine, double * beta, int64_t row_stride,
                              int64_t columns, int32_t grid, int32_t n_paths,
                              int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                              const double * level_table, double diffusivity,
                              const double * view_cosine, const double * surface_temperature,
                              const double * emissivity_rows, const double * emissivity,
                              const double * up_rows, const double * down_rows, int32_t n_bands,
                              const int64_t * band_start, double * radiance_rows,
                              double * brightness_rows, double * radiance_mean, int32_t flags)
{
    return path_thermal_radiance(
        engine, "lbl_path_thermal_radiance", beta, row_stride, columns, grid, n_paths,
        levels_per_path, level_begin, level_count, level_table, nullptr, false, nullptr,
        diffusivity, view_cosine, surface_temperature, emissivity_rows, emissivity, up_rows,
        down_rows, n_bands, band_start, radiance_rows, brightness_rows, radiance_mean, flags);
}

int lbl_path_thermal_radiance_source(
    lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns, int32_t grid,
    int32_t n_paths, int32_t levels_per_path, int32_t level_begin, int32_t level_count,
    const double * level_table, const double * edge_temperature, double diffusivity,
    const double * view_cosine, const double * surface_temperature,
    const double * emissivity_rows, const double * emissivity, const double * up_rows,
    const double * down_rows, int32_t n_bands, const int64_t * band_start,
    double * radiance_rows, double * brightness_rows, double * radiance_mean, int32_t flags)
{
    return path_thermal_radiance(
        engine, "lbl_path_thermal_radiance_source", beta, row_stride, columns, grid, n_paths,
        levels_per_path, level_begin, level_count, level_table, edge_temperature, true, nullptr,
        diffusivity, view_cosine, surface_temperature, emissivity_rows, emissivity, up_rows,
        down_rows, n_bands, band_start, radiance_rows, brightness_rows, radiance_mean, flags);
}

int lbl_path_thermal_radiance_spectral(
    lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns, int32_t grid,
    int32_t n_paths, int32_t levels_per_path, int32_t level_begin, int32_t level_count,
    const double * level_table, int32_t n_knots, const double * knot_wavenumber,
    const double * knot_optics, double diffusivity, const double * view_cosine,
    const double * surface_temperature, const double * emissivity_rows, const double * emissivity,
    const double * up_rows, const double * down_rows, int32_t n_bands,
    const int64_t * band_start, double * radiance_rows, double * brightness_rows,
    double * radiance_mean, int32_t flags)
{
    ScattererTable spectral{n_knots, knot_wavenumber, knot_optics};
    return path_thermal_radiance(
        engine, "lbl_path_thermal_radiance_spectral", beta, row_stride, columns, grid, n_paths,
        levels_per_path, level_begin, level_count, level_table, nullptr, false, &spectral,
        diffusivity, view_cosine, surface_temperature, emissivity_rows, emissivity, up_rows,
        down_rows, n_bands, band_start, radiance_rows, brightness_rows, radiance_mean, flags);
}

}  // extern "C"
