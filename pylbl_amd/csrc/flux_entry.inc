// lbl_path_flux_source: one sweep (down from space or up from the surface) of K angles through a
// block of absorption coefficients in HBM (kernel: flux.h; band means: path.h), and
// lbl_path_flux, the same call without edge temperatures.  Included by engine.hip
// after radiance_entry.inc; shares path_entry.inc's PathCall, PathTables and PathBands.
extern "C" {

int lbl_path_flux_source(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                         int32_t grid, int32_t n_paths, int32_t levels_per_path,
                         int32_t level_begin, int32_t level_count, int32_t n_angles,
                         const double * path_length, const double * weight,
                         const double * temperature, const double * edge_temperature,
                         const double * surface_temperature, const double * surface_emissivity,
                         int32_t n_bands, const int64_t * band_start, double * carry,
                         double * reflection, double * level_flux, double * flux,
                         double * surface_flux, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_path_flux_source", row_stride, columns, n_paths, levels_per_path,
                      level_begin, level_count, flags};
        const bool up = (flags & LBL_PATH_FLUX_UP) != 0;
        if (beta == nullptr || path_length == nullptr || weight == nullptr ||
            temperature == nullptr || carry == nullptr || reflection == nullptr ||
            level_flux == nullptr)
        {
            return call.bad("beta, path_length, weight, temperature, carry, reflection and "
                            "level_flux must not be NULL.");
        }
        if (level_flux == beta)
        {
            return call.bad("level_flux must not be beta: the up sweep reads it.");
        }
        if (up && (surface_temperature == nullptr || surface_emissivity == nullptr))
        {
            return call.bad("the up sweep needs surface_temperature and surface_emissivity.");
        }
        if (n_angles < 1 || n_angles > kFluxMaxAngles) return call.bad("need 1 <= n_angles <= 8.");
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        if (const char * problem = call.check(path_length, n_angles)) return call.bad(problem);
        if (!finite_at_least_zero(weight, n_angles, false))
        {
            return call.bad("weights must be finite and >= 0.");
        }
        if (!finite_at_least_zero(temperature, level_count, true))
        {
            return call.bad("temperatures must be finite and > 0.");
        }
        if (const char * problem = check_edge_temperatures(edge_temperature, level_begin,
                                                           level_count, levels_per_path))
        {
            return call.bad(problem);
        }
        if (up)
        {
            for (int p = 0; p < n_paths; ++p)
            {
                if (!(surface_temperature[p] > 0.) || !std::isfinite(surface_temperature[p]))
                {
                    return call.bad("surface temperatures must be finite and > 0.");
                }
                if (!(surface_emissivity[p] >= 0. && surface_emissivity[p] <= 1.))
                {
                    return call.bad("surface emissivities must lie in [0, 1].");
                }
            }
        }
        PathBands bands;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }
        if (n_bands > 0 && (flux == nullptr || (up && surface_flux == nullptr)))
        {
            return call.bad("band means need flux (and surface_flux on the up sweep).");
        }

        // The surface temperatures and emissivities of the run's paths (0 on the down sweep).
        const PathRun & run = call.run;
        PathTables tables;
        const size_t length_at = tables.add((size_t)level_count*n_angles, path_length);
        const size_t weight_at = tables.add(n_angles, weight);
        const size_t temperature_at = tables.add(level_count, temperature);
        const size_t surface_at = tables.add_pair(run, up ? surface_temperature : nullptr, 0.,
                                                  up ? surface_emissivity : nullptr, 0.);
        tables.add(bands, band_start);
        // After the tables every call has, so that theirs lie where they always lay.
        const bool linear = edge_temperature != nullptr;
        const size_t edge_at = linear ? tables.add(2*(size_t)level_count, edge_temperature) : 0;
        const double * d_tables = call.begin(tables);

        PathFlux a;
        call.fill(a, beta, carry);
        a.nu = call.grid->wavenumber.data;
        a.length = d_tables + length_at;
        a.weight = d_tables + weight_at;
        a.temperature = d_tables + temperature_at;
        a.surface_t = d_tables + surface_at;
        a.surface_e = a.surface_t + run.paths;
        a.edge = linear ? d_tables + edge_at : nullptr;
        a.table_path = run.first_path;
        a.up = up ? 1 : 0;
        a.reflection = reflection;
        a.level_flux = level_flux;
        const bool vector = path_vector(row_stride, {beta, carry, a.nu, reflection, level_flux});
        call.launch(a, [&](const dim3 & launch) {
            // (1 <= n_angles <= kFluxMaxAngles was checked above: one of them is launched)
            dispatch_range<kFluxMaxAngles>([&](auto k, auto v, auto l) {
                hipLaunchKernelGGL((path_flux_kernel<v.value, k.value, l.value>), launch,
                                   dim3(kPathThreads), 0, engine->stream, a);
            }, n_angles, vector, linear);
        });
        call.note_rows(beta, level_count);
        call.note_rows(level_flux, level_count);
        call.note_rows(carry, (long long)n_paths*n_angles);
        call.note_rows(reflection, n_paths);

        // Every interface of the run, and the surface-interface rows of the paths it starts.
        call.means(bands, PathMeanRows::kLevels, level_flux, flux);
        call.means(bands, PathMeanRows::kStarted, reflection, up ? surface_flux : nullptr);
        return LBL_OK;
    });
}

int lbl_path_flux(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                  int32_t grid, int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                  int32_t level_count, int32_t n_angles, const double * path_length,
                  const double * weight, const double * temperature,
                  const double * surface_temperature, const double * surface_emissivity,
                  int32_t n_bands, const int64_t * band_start, double * carry,
                  double * reflection, double * level_flux, double * flux, double * surface_flux,
                  int32_t flags)
{
    return lbl_path_flux_source(engine, beta, row_stride, columns, grid, n_paths, levels_per_path,
                                level_begin, level_count, n_angles, path_length, weight,
                                temperature, nullptr, surface_temperature, surface_emissivity,
                                n_bands, band_start, carry, reflection, level_flux, flux,
                                surface_flux, flags);
}

}  // extern "C"
