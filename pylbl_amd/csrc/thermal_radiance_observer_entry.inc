// lbl_path_thermal_radiance_observer (include/lbl_amd_thermal_radiance_observer.h): the radiance
// through clouds at an observer after n_p levels of each path, looking down or up, from the
// two-stream fluxes lbl_path_thermal_two_stream or, with an edge table,
// lbl_path_thermal_two_stream_source left in HBM (kernel: thermal_radiance_observer.h; band means:
// path.h).  Included by engine.hip after thermal_radiance_entry.inc, whose checks it repeats in
// their order; shares path_entry.inc's PathCall, TwoStreamCall, PathTables, PathBands and
// check_edge_temperatures.
extern "C" {

int lbl_path_thermal_radiance_observer(
    lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns, int32_t grid,
    int32_t n_paths, int32_t levels_per_path, int32_t level_begin, int32_t level_count,
    const double * level_table, const double * edge_temperature, double diffusivity,
    const double * view_cosine, const int32_t * observer_levels, int32_t view_up,
    const double * surface_temperature, const double * emissivity_rows, const double * emissivity,
    const double * up_rows, const double * down_rows, int32_t n_bands,
    const int64_t * band_start, double * radiance_rows, double * brightness_rows,
    double * radiance_mean, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_path_thermal_radiance_observer", row_stride, columns, n_paths,
                      levels_per_path, level_begin, level_count, flags};
        double * const rows[2] = {radiance_rows, brightness_rows};
        double * const mean[2] = {radiance_mean, nullptr};
        const TwoStreamCall two{call, 2, 0, rows, mean};
        const bool linear = edge_temperature != nullptr;
        if (beta == nullptr || level_table == nullptr || view_cosine == nullptr ||
            observer_levels == nullptr || surface_temperature == nullptr)
        {
            return call.bad("beta, level_table, view_cosine, observer_levels and "
                            "surface_temperature must not be NULL.");
        }
        if (view_up != 0 && view_up != 1) return call.bad("view_up must be 0 or 1.");
        if ((emissivity_rows == nullptr) == (emissivity == nullptr))
        {
            return call.bad("the surface needs an emissivity: emissivity_rows or emissivity, not "
                            "both.");
        }
        if (up_rows == nullptr || down_rows == nullptr)
        {
            return call.bad("up_rows and down_rows, the fluxes of lbl_path_thermal_two_stream or "
                            "lbl_path_thermal_two_stream_source, must not be NULL.");
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
        // The surface is checked looking up too, although that sweep does not read it.
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
            if (observer_levels[p] < 0 || observer_levels[p] > levels_per_path)
            {
                return call.bad("observer_levels must lie in [0, levels_per_path].");
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
        const size_t mu_at = tables.add(run.paths, view_cosine + run.first_path);
        // n_p as a double: a whole number below 2^31 is exact.
        const size_t observer_at = tables.add(run.paths);
        for (int i = 0; i < run.paths; ++i)
        {
            tables.words[observer_at + (size_t)i] = (double)observer_levels[run.first_path + i];
        }
        tables.add(bands, band_start);
        const size_t edge_at = tables.add(linear ? 2*(size_t)level_count : 0, edge_temperature);
        const double * d_tables = call.begin(tables);

        const double * nu = call.grid->wavenumber.data;
        const bool vector = path_vector(row_stride, {beta, nu, emissivity_rows, up_rows,
                                                     down_rows, radiance_rows, brightness_rows});
        PathThermalObserver a;
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
        a.observer = d_tables + observer_at;
        a.up = up_rows;
        a.down = down_rows;
        a.rad = radiance_rows;
        a.bt = brightness_rows;
        // Space -> surface is from_last() (the surface is level 0); looking down runs against it.
        const int down_order = call.from_last() ? 1 : 0;
        a.from_last = view_up ? down_order : 1 - down_order;
        dispatch([&](auto source, auto up) {
            two.sweep(a, vector, [](auto v) {
                return thermal_observer_kernel<decltype(v)::value, decltype(source)::value,
                                               decltype(up)::value>;
            });
        }, linear, view_up != 0);
        call.note_rows(beta, level_count);
        call.note_rows(up_rows, level_count);
        call.note_rows(down_rows, level_count);
        call.note_rows(radiance_rows, n_paths);
        call.note_rows(brightness_rows, n_paths);
        call.means(bands, PathMeanRows::kStarted, radiance_rows, radiance_mean);
        return LBL_OK;
    });
}

}  // extern "C"
