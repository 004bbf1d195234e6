// lbl_path_radiance_source: thermal emission along paths through a block of absorption
// coefficients in HBM (kernel: radiance.h; band means: path.h), and lbl_path_radiance, the same
// call without edge temperatures.  Included by engine.hip after path_entry.inc,
// whose PathCall, PathTables and PathBands it shares.
extern "C" {

int lbl_path_radiance_source(lbl_engine * engine, double * beta, int64_t row_stride,
                             int64_t columns, int32_t grid, int32_t n_paths,
                             int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                             const double * path_length, const double * temperature,
                             const double * edge_temperature,
                             const double * boundary_temperature,
                             const double * boundary_emissivity, int32_t n_bands,
                             const int64_t * band_start, double * carry, double * radiance,
                             double * brightness_temperature, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_path_radiance_source", row_stride, columns, n_paths, levels_per_path,
                      level_begin, level_count, flags};
        const bool want_rad = (flags & LBL_PATH_RADIANCE) != 0;
        const bool want_bt = (flags & LBL_PATH_BRIGHTNESS) != 0;
        const bool cumulative = (flags & LBL_PATH_CUMULATIVE) != 0;
        if (beta == nullptr || path_length == nullptr || temperature == nullptr ||
            carry == nullptr)
        {
            return call.bad("beta, path_length, temperature and carry must not be NULL.");
        }
        if (!want_rad && !want_bt) return call.bad("no quantity requested.");
        if ((want_rad && radiance == nullptr) || (want_bt && brightness_temperature == nullptr))
        {
            return call.bad("an output requested by the flags is NULL.");
        }
        if (want_bt && n_bands != 0) return call.bad("brightness temperature has no band means.");
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        if (const char * problem = call.check(path_length, 1)) return call.bad(problem);
        if (!finite_at_least_zero(temperature, level_count, true))
        {
            return call.bad("temperatures must be finite and > 0.");
        }
        if (edge_temperature != nullptr)
        {
            if (const char * problem = check_edge_temperatures(edge_temperature, level_begin,
                                                               level_count, levels_per_path))
            {
                return call.bad(problem);
            }
        }
        for (int p = 0; p < n_paths; ++p)
        {
            const double t = boundary_temperature != nullptr ? boundary_temperature[p] : 0.;
            const double e = boundary_emissivity != nullptr ? boundary_emissivity[p] : 1.;
            if (!(t >= 0.) || !std::isfinite(t))
            {
                return call.bad("boundary temperatures must be finite and >= 0 (0: no boundary).");
            }
            if (!(e >= 0. && e <= 1.)) return call.bad("boundary emissivities must lie in [0, 1].");
        }
        PathBands bands;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }

        // The boundary temperatures and emissivities of the run's paths.
        const PathRun & run = call.run;
        PathTables tables;
        const size_t length_at = tables.add(level_count, path_length);
        const size_t temperature_at = tables.add(level_count, temperature);
        const size_t boundary_at = tables.add(2*(size_t)run.paths);
        double * boundary = tables.words.data() + boundary_at;
        for (int i = 0; i < run.paths; ++i)
        {
            const int p = run.first_path + i;
            boundary[i] = boundary_temperature != nullptr ? boundary_temperature[p] : 0.;
            boundary[run.paths + i] = boundary_emissivity != nullptr ? boundary_emissivity[p] : 1.;
        }
        const size_t band_at = tables.add(bands, band_start);
        // After the tables every call has, so that theirs lie where they always lay.
        const bool linear = edge_temperature != nullptr;
        const size_t edge_at = linear ? tables.add(2*(size_t)level_count, edge_temperature) : 0;
        const double * d_tables = call.begin(tables);

        PathRadiance a;
        a.beta = beta;
        a.stride = row_stride;
        a.columns = columns;
        a.nu = call.grid->wavenumber.data;
        a.length = d_tables + length_at;
        a.temperature = d_tables + temperature_at;
        a.boundary_t = d_tables + boundary_at;
        a.boundary_e = a.boundary_t + run.paths;
        a.edge = linear ? d_tables + edge_at : nullptr;
        a.first = level_begin;
        a.count = level_count;
        a.row_base = level_begin;
        a.levels_per_path = levels_per_path;
        a.table_path = run.first_path;
        a.from_last = call.from_last() ? 1 : 0;
        a.carry = carry;
        a.level_rad = a.level_bt = a.final_rad = a.final_bt = nullptr;
        a.keep_final = 0;
        if (cumulative && n_bands > 0)
        {
            a.level_rad = beta;         // in place: the band means read the rows back
        }
        else if (cumulative)
        {
            a.level_rad = want_rad ? radiance : nullptr;
            a.level_bt = want_bt ? brightness_temperature : nullptr;
        }
        else if (n_bands > 0)
        {
            a.keep_final = 1;
        }
        else
        {
            a.final_rad = want_rad ? radiance : nullptr;
            a.final_bt = want_bt ? brightness_temperature : nullptr;
        }
        const bool vector = path_vector(row_stride, {beta, carry, a.nu, a.level_rad, a.level_bt,
                                                     a.final_rad, a.final_bt});
        call.launch([&](const dim3 & launch, int first_path) {
            a.first_path = first_path;
            if (vector && linear)
            {
                hipLaunchKernelGGL((path_radiance_kernel<true, true>), launch,
                                   dim3(kPathThreads), 0, engine->stream, a);
            }
            else if (linear)
            {
                hipLaunchKernelGGL((path_radiance_kernel<false, true>), launch,
                                   dim3(kPathThreads), 0, engine->stream, a);
            }
            else if (vector)
            {
                hipLaunchKernelGGL(path_radiance_kernel<true>, launch, dim3(kPathThreads), 0,
                                   engine->stream, a);
            }
            else
            {
                hipLaunchKernelGGL(path_radiance_kernel<false>, launch, dim3(kPathThreads), 0,
                                   engine->stream, a);
            }
        });
        call.note_rows(beta, level_count);
        call.note_rows(a.level_rad != beta ? a.level_rad : nullptr, level_count);
        call.note_rows(a.level_bt, level_count);
        call.note_rows(carry, n_paths);
        call.note_rows(a.final_rad, n_paths);
        call.note_rows(a.final_bt, n_paths);

        if (n_bands > 0)
        {
            // Rows: every level of the run (cumulative, in place in beta) or the paths the run
            // finishes -- upward those whose last level is in the run, downward those whose
            // first level is -- from their carry rows.
            const PathRows rows = cumulative ? PathRows{0, level_count}
                                             : path_rows(level_begin, call.level_end(),
                                                         levels_per_path, !call.from_last());
            const double * values = cumulative ? beta : carry + (long long)rows.first*row_stride;
            double * out = radiance + (cumulative ? 0 : (long long)rows.first*n_bands);
            bands.means(engine, reinterpret_cast<const long long *>(d_tables + band_at), values,
                        (long long)row_stride, rows.count, false, out);
        }
        return LBL_OK;
    });
}

int lbl_path_radiance(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                      int32_t grid, int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                      int32_t level_count, const double * path_length, const double * temperature,
                      const double * boundary_temperature, const double * boundary_emissivity,
                      int32_t n_bands, const int64_t * band_start, double * carry,
                      double * radiance, double * brightness_temperature, int32_t flags)
{
    return lbl_path_radiance_source(engine, beta, row_stride, columns, grid, n_paths,
                                    levels_per_path, level_begin, level_count, path_length,
                                    temperature, nullptr, boundary_temperature,
                                    boundary_emissivity, n_bands, band_start, carry, radiance,
                                    brightness_temperature, flags);
}

}  // extern "C"
