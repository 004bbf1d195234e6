// lbl_path_thermal_two_stream and lbl_path_thermal_two_stream_source: two-stream longwave fluxes
// at every interface of whole paths through a block of absorption coefficients in HBM, with one
// grey scatterer per level; the second with a source that is linear in optical depth between the
// Planck values at every level's two interfaces (kernels: twostream_thermal.h; band means:
// path.h); lbl_path_thermal_two_stream_spectral: either source with the scatterer of every level
// as a table over wavenumber (include/lbl_amd_scatterer.h; kernels: scatterer.h).  Included by
// engine.hip after twostream_entry.inc; shares path_entry.inc's PathCall, TwoStreamCall,
// PathTables, PathBands and check_edge_temperatures, and twostream_entry.inc's ScattererTable.
namespace {

// All three entries.  name: the entry's; edge_temperature: [level_count][2], or null for the
// source of the level temperatures; spectral: the scatterer's knot table, or null for the grey
// scatterer of the level table.
int path_thermal_two_stream(lbl_engine * engine, const char * name, double * beta,
                            int64_t row_stride, int64_t columns, int32_t grid, int32_t n_paths,
                            int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                            const double * level_table, const double * edge_temperature,
                            bool linear, ScattererTable * spectral, double diffusivity,
                            const double * surface_temperature,
                            const double * emissivity_rows, const double * emissivity,
                            int32_t n_bands, const int64_t * band_start, double * work,
                            double * const (&rows)[4], double * const (&mean)[4], int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, name, row_stride, columns, n_paths, levels_per_path, level_begin,
                      level_count, flags};
        // Up, down: below each level, then at interface 0 of each path.
        constexpr int kRows = 4, kPerLevel = 2;
        const TwoStreamCall two{call, kRows, kPerLevel, rows, mean};
        if (beta == nullptr || level_table == nullptr || (linear && edge_temperature == nullptr) ||
            surface_temperature == nullptr || work == nullptr)
        {
            return call.bad(linear ? "beta, level_table, edge_temperature, surface_temperature "
                                     "and work must not be NULL."
                                   : "beta, level_table, surface_temperature and work must not be "
                                     "NULL.");
        }
        if ((emissivity_rows == nullptr) == (emissivity == nullptr))
        {
            return call.bad("the surface needs an emissivity: emissivity_rows or emissivity, not "
                            "both.");
        }
        if (const char * problem = two.check_whole_paths()) return call.bad(problem);
        if (const char * problem = two.check_outputs(beta, work, n_bands))
        {
            return call.bad(problem);
        }
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
        tables.add(bands, band_start);
        const size_t edge_at = tables.add(linear ? 2*(size_t)level_count : 0, edge_temperature);
        if (spectral != nullptr) spectral->stage(tables, level_count);
        const double * d_tables = call.begin(tables);

        PathThermalSpectral a;
        call.fill(a, beta, nullptr);
        a.nu = call.grid->wavenumber.data;
        a.level = d_tables + level_at;
        a.diffusivity = diffusivity;
        a.surface_t = d_tables + ts_at;
        a.surface_e = d_tables + eps_at;
        a.table_path = run.first_path;
        a.emissivity_rows = emissivity_rows;
        a.work = work;
        a.edge = linear ? d_tables + edge_at : nullptr;
        for (int q = 0; q < kPerLevel; ++q)
        {
            a.level_out[q] = rows[q];
            a.top_out[q] = rows[kPerLevel + q];
        }
        const bool vector = path_vector(row_stride, {beta, a.nu, emissivity_rows, work, rows[0],
                                                     rows[1], rows[2], rows[3]});
        if (spectral != nullptr)
        {
            a.scatterer = spectral->on_device(d_tables, a.nu);
            a.scatters = d_tables + spectral->scatters_at;
        }
        dispatch([&](auto source, auto knots) {
            constexpr bool kLinear = decltype(source)::value;
            constexpr bool kSpectral = decltype(knots)::value;
            ThermalArguments<kSpectral> & arguments = a;
            two.sweeps(arguments, vector,
                       [](auto v) {
                           return thermal_up_kernel<decltype(v)::value, kLinear, kSpectral>;
                       },
                       [](auto v) {
                           return thermal_down_kernel<decltype(v)::value, kLinear, kSpectral>;
                       });
        }, linear, spectral != nullptr);
        two.finish(bands, beta, work);
        return LBL_OK;
    });
}

}  // namespace

extern "C" {

int lbl_path_thermal_two_stream(lbl_engine * engine, double * beta, int64_t row_stride,
                                int64_t columns, int32_t grid, int32_t n_paths,
                                int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                                const double * level_table, double diffusivity,
                                const double * surface_temperature,
                                const double * emissivity_rows, const double * emissivity,
                                int32_t n_bands, const int64_t * band_start, double * work,
                                double * up_rows, double * down_rows, double * top_up_rows,
                                double * top_down_rows, double * up_mean, double * down_mean,
                                double * top_up_mean, double * top_down_mean, int32_t flags)
{
    return path_thermal_two_stream(
        engine, "lbl_path_thermal_two_stream", beta, row_stride, columns, grid, n_paths,
        levels_per_path, level_begin, level_count, level_table, nullptr, false, nullptr,
        diffusivity,
        surface_temperature, emissivity_rows, emissivity, n_bands, band_start, work,
        {up_rows, down_rows, top_up_rows, top_down_rows},
        {up_mean, down_mean, top_up_mean, top_down_mean}, flags);
}

int lbl_path_thermal_two_stream_source(
    lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns, int32_t grid,
    int32_t n_paths, int32_t levels_per_path, int32_t level_begin, int32_t level_count,
    const double * level_table, const double * edge_temperature, double diffusivity,
    const double * surface_temperature, const double * emissivity_rows, const double * emissivity,
    int32_t n_bands, const int64_t * band_start, double * work, double * up_rows,
    double * down_rows, double * top_up_rows, double * top_down_rows, double * up_mean,
    double * down_mean, double * top_up_mean, double * top_down_mean, int32_t flags)
{
    return path_thermal_two_stream(
        engine, "lbl_path_thermal_two_stream_source", beta, row_stride, columns, grid, n_paths,
        levels_per_path, level_begin, level_count, level_table, edge_temperature, true, nullptr,
        diffusivity, surface_temperature, emissivity_rows, emissivity, n_bands, band_start, work,
        {up_rows, down_rows, top_up_rows, top_down_rows},
        {up_mean, down_mean, top_up_mean, top_down_mean}, flags);
}

int lbl_path_thermal_two_stream_spectral(
    lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns, int32_t grid,
    int32_t n_paths, int32_t levels_per_path, int32_t level_begin, int32_t level_count,
    const double * level_table, const double * edge_temperature, int32_t n_knots,
    const double * knot_wavenumber, const double * knot_optics, double diffusivity,
    const double * surface_temperature, const double * emissivity_rows, const double * emissivity,
    int32_t n_bands, const int64_t * band_start, double * work, double * up_rows,
    double * down_rows, double * top_up_rows, double * top_down_rows, double * up_mean,
    double * down_mean, double * top_up_mean, double * top_down_mean, int32_t flags)
{
    ScattererTable spectral{n_knots, knot_wavenumber, knot_optics};
    return path_thermal_two_stream(
        engine, "lbl_path_thermal_two_stream_spectral", beta, row_stride, columns, grid, n_paths,
        levels_per_path, level_begin, level_count, level_table, edge_temperature,
        edge_temperature != nullptr, &spectral, diffusivity, surface_temperature, emissivity_rows,
        emissivity, n_bands, band_start, work, {up_rows, down_rows, top_up_rows, top_down_rows},
        {up_mean, down_mean, top_up_mean, top_down_mean}, flags);
}

}  // extern "C"
