// lbl_path_thermal_two_stream_source: lbl_path_thermal_two_stream with a source that is linear in
// optical depth between the Planck values at every level's two interfaces (kernels:
// twostream_thermal_source.h; band means: path.h).  Included by engine.hip after
// thermal_entry.inc; shares path_entry.inc's PathCall, PathTables, PathBands and
// check_edge_temperatures.
extern "C" {

int lbl_path_thermal_two_stream_source(
    lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns, int32_t grid,
    int32_t n_paths, int32_t levels_per_path, int32_t level_begin, int32_t level_count,
    const double * level_table, const double * edge_temperature, double diffusivity,
    const double * surface_temperature, const double * emissivity_rows, const double * emissivity,
    int32_t n_bands, const int64_t * band_start, double * work, double * up_rows,
    double * down_rows, double * top_up_rows, double * top_down_rows, double * up_mean,
    double * down_mean, double * top_up_mean, double * top_down_mean, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_path_thermal_two_stream_source", row_stride, columns, n_paths,
                      levels_per_path, level_begin, level_count, flags};
        // Up, down: below each level, then at interface 0 of each path.
        constexpr int kRows = 4, kPerLevel = 2;
        double * const rows[kRows] = {up_rows, down_rows, top_up_rows, top_down_rows};
        double * const mean[kRows] = {up_mean, down_mean, top_up_mean, top_down_mean};
        if (beta == nullptr || level_table == nullptr || edge_temperature == nullptr ||
            surface_temperature == nullptr || work == nullptr)
        {
            return call.bad("beta, level_table, edge_temperature, surface_temperature and work "
                            "must not be NULL.");
        }
        if ((emissivity_rows == nullptr) == (emissivity == nullptr))
        {
            return call.bad("the surface needs an emissivity: emissivity_rows or emissivity, not "
                            "both.");
        }
        if (flags & ~(LBL_PATH_FROM_LAST | LBL_ASYNC))
        {
            return call.bad("only LBL_PATH_FROM_LAST and LBL_ASYNC may be set: a call takes "
                            "whole paths.");
        }
        if (levels_per_path >= 1 &&
            (level_begin % levels_per_path != 0 || level_count % levels_per_path != 0))
        {
            return call.bad("the run must consist of whole paths: level_begin and level_count "
                            "must be multiples of levels_per_path.");
        }
        bool any = false;
        for (int q = 0; q < kRows; ++q)
        {
            any = any || rows[q] != nullptr;
            if (rows[q] != nullptr && (rows[q] == beta || rows[q] == work))
            {
                return call.bad("an output must be neither beta nor the work rows.");
            }
            if (mean[q] != nullptr && rows[q] == nullptr)
            {
                return call.bad("a band mean needs the rows it is the mean of.");
            }
            if (mean[q] != nullptr && n_bands == 0) return call.bad("band means need n_bands > 0.");
        }
        if (!any) return call.bad("no output requested.");
        if (work == beta) return call.bad("work must not be beta.");
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        // The thicknesses are the run's lengths; the other four columns of the table follow.
        if (level_count < 1) return call.bad("need level_count >= 1.");
        {
            std::vector<double> thickness((size_t)level_count);
            for (int r = 0; r < level_count; ++r)
            {
                thickness[(size_t)r] = level_table[(size_t)r*kThermalLevelWords];
            }
            if (const char * problem = call.check(thickness.data(), 1)) return call.bad(problem);
        }
        if (!finite_at_least_zero(level_table, (long long)level_count*kThermalLevelWords, false))
        {
            return call.bad("the level table must be finite and >= 0.");
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

        const PathRun & run = call.run;
        PathTables tables;
        const size_t level_at = tables.add((size_t)level_count*kThermalLevelWords, level_table);
        const size_t ts_at = tables.add(run.paths, surface_temperature + run.first_path);
        const size_t eps_at =
            tables.add(run.paths, emissivity != nullptr ? emissivity + run.first_path : nullptr);
        tables.add(bands, band_start);
        const size_t edge_at = tables.add(2*(size_t)level_count, edge_temperature);
        const double * d_tables = call.begin(tables);

        PathThermalSource a;
        call.fill(a, beta, nullptr);
        a.nu = call.grid->wavenumber.data;
        a.level = d_tables + level_at;
        a.diffusivity = diffusivity;
        a.surface_t = d_tables + ts_at;
        a.surface_e = d_tables + eps_at;
        a.table_path = run.first_path;
        a.emissivity_rows = emissivity_rows;
        a.work = work;
        a.edge = d_tables + edge_at;
        for (int q = 0; q < kPerLevel; ++q)
        {
            a.level_out[q] = rows[q];
            a.top_out[q] = rows[kPerLevel + q];
        }
        const bool vector = path_vector(row_stride, {beta, a.nu, emissivity_rows, work, rows[0],
                                                     rows[1], rows[2], rows[3]});
        // Up from the surface, then down from space behind it on the same stream.  The order
        // space -> surface is from_last() (the surface is level 0); the up sweep runs against it.
        const int down_order = call.from_last() ? 1 : 0;
        a.from_last = 1 - down_order;
        call.launch(a, [&](const dim3 & launch) {
            dispatch([&](auto v) {
                hipLaunchKernelGGL(thermal_source_up_kernel<v.value>, launch, dim3(kPathThreads),
                                   0, engine->stream, a);
            }, vector);
        });
        a.from_last = down_order;
        call.launch(a, [&](const dim3 & launch) {
            dispatch([&](auto v) {
                hipLaunchKernelGGL(thermal_source_down_kernel<v.value>, launch,
                                   dim3(kPathThreads), 0, engine->stream, a);
            }, vector);
        });
        call.note_rows(beta, level_count);
        call.note_rows(work, 2*(long long)level_count);
        for (int q = 0; q < kRows; ++q)
        {
            call.note_rows(rows[q], q < kPerLevel ? level_count : n_paths);
        }

        // Every interface below a level of the run; interface 0 of its (whole) paths.
        for (int q = 0; q < kRows; ++q)
        {
            call.means(bands, q < kPerLevel ? PathMeanRows::kLevels : PathMeanRows::kStarted,
                       rows[q], mean[q]);
        }
        return LBL_OK;
    });
}

}  // extern "C"
